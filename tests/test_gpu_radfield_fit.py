"""The radiation-field fit on the device (artis_amd_radfield_*) against the x86 build of the same rules (tests/radfield_host)
applied to the downloaded estimators and cell state, after a few resident timesteps of the synthetic models. Per-cell values,
normalised estimators and bin counts are identical; a float that the device's pow / exp moves by one ulp is allowed and counted;
bin T_R agrees to 1e-4 (the root search's tolerance) and W matches the host integral at the device's T_R."""
import numpy as np
import pytest

import test_radfield_fit_rules as rules
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
WIDTH = 0.05


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


def _run(engine_mod, preset, nsteps=2, npk=20000, thick_below_v=0.0):
    model, cs0, _, aux = synth.build("small", ncoord=8, options=preset, nts=10, thick_below_v=thick_below_v)
    pk0 = synth.make_packets(model, aux, npk, kpkt_fraction=0.2, ts_width_frac=(1.0 + WIDTH) ** nsteps - 1.0)
    eng = engine_mod.Engine(model, preset=preset)
    eng.upload_packets(pk0)
    t = aux["t"]
    for i in range(nsteps):
        ts = synth.make_timestep(t, width_frac=WIDTH, vmax=model["vmax"], nts=10 + i)
        cs = synth.evolve_cellstate(cs0, aux["t"], ts.c.mid)
        eng.set_cellstate(cs, ts)
        eng.step()
        t = ts.c.start + ts.c.width
    return eng, model, cs, ts


def _download(eng, model, info):
    n = model["npts_nonempty"]
    est = abi.Estimators(n, model["nbfcontinua_ground"], nbfcontinua=max(info["nbfestim"], 1) if info["extended"] else 0,
                         nbins=max(info["nbins"], 1), ndetailedlines=info["nline"])
    eng.download_estimators(est)
    return est


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _compare(eng, model, cs, ts, preset, lte=False, seed=None, nprocs=1):
    vol = synth.assocvolume_tmin(model)
    prev_mid, deltat = ts.c.mid, ts.c.width
    d = eng.radfield_fit(prev_mid, deltat, vol, nprocs=nprocs, lte_iteration=lte, bfrate_normed_seed=seed)
    nb = d["radfieldbin_T_R"].shape[1] if "radfieldbin_T_R" in d else 0
    nbf = len(d["bfrate_normed"]) // model["npts_nonempty"] if "bfrate_normed" in d else 0
    nline = len(d["Jb_lu_normed"]) // model["npts_nonempty"] if "Jb_lu_normed" in d else 0
    info = dict(nbins=nb, nbfestim=nbf, nline=nline, extended=preset in abi.NEBULAR_FAMILY)
    est = _download(eng, model, info)
    bf_state = np.zeros(max(model["npts_nonempty"] * nbf, 1), np.float32)
    if seed is not None:
        bf_state[: len(seed)] = seed
    h = rules.host_fit(preset, model, dict(cs.d), est, prev_mid, deltat, vol, nprocs=nprocs, lte=lte, nbf=nbf, nline=nline,
                       bf_state=bf_state, nthreads=16)
    for k in ("J", "nuJ", "J_normfactor", "flags", "cell_counts"):
        assert np.array_equal(d[k], h[k]), k
    nulp = 0
    for k in ("TJ", "TR", "Te", "W"):
        u = _ulps(d[k], h[k])
        assert u.max() <= 1, (k, int(u.max()))
        nulp += int((u == 1).sum())
    print(f"{preset}: {nulp} per-cell floats 1 ulp apart of {4 * model['npts_nonempty']}")
    assert d["totals"] == h["totals"]
    if nbf:
        assert np.array_equal(d["bfrate_normed"], h["bfrate_normed"])
    if nline:
        assert np.array_equal(d["Jb_lu_normed"], h["Jb_lu_normed"])
        assert np.array_equal(d["Jb_lu_contribcount"], h["Jb_lu_contribcount"])
    if nb:
        L = rules.lib(preset)
        lo, hi = rules.bin_edges(preset)
        Td, Th, Wd = d["radfieldbin_T_R"], h["radfieldbin_T_R"], d["radfieldbin_W"]
        same = int(np.sum((Td == Th) & (Wd == h["radfieldbin_W"])))
        fitted = (d["flags"] & abi.RADFIELD_FITTED) != 0
        nf = d["J_normfactor"]
        Jb = est.radfieldbin_J.reshape(-1, nb) * nf[:, None]
        nuJb = est.radfieldbin_nuJ.reshape(-1, nb) * nf[:, None]
        # T_R agrees to the root search's tolerance, except where the residual is flatter than its own rounding: in a narrow bin at
        # small x the Planck mean frequency hardly moves with T_R, and a last-bit difference of the device's exp moves the root
        # further. There the device's T_R must still bracket nu_bar to within that rounding (as tests/test_radfield_fit_rules.py
        # checks of the host's).
        rel = np.abs(Td - Th) / np.maximum(np.abs(Th), 1.0)
        far = np.argwhere(rel > 1e-4)
        for c, b in far:
            T_R, J_bin = float(Td[c, b]), Jb[c, b]
            assert 500 < T_R < 250000 and J_bin > 0, (c, b, T_R, float(Th[c, b]))
            nubar = nuJb[c, b] / J_bin
            xl, xh = rules.H * lo[b] / (rules.KB * T_R), rules.H * hi[b] / (rules.KB * T_R)
            cancel = L.rf_host_partial(xl, 0) / (L.rf_host_partial(xl, 0) - L.rf_host_partial(xh, 0)) if xl < 100 else 1.0
            slack = (1e-13 if xl >= 0.03 else 1e-9) * cancel * nubar
            assert (L.rf_host_mean_frequency(T_R * (1 - 1.01e-4), lo[b], hi[b]) - slack <= nubar
                    <= L.rf_host_mean_frequency(T_R * (1 + 1.01e-4), lo[b], hi[b]) + slack), (c, b, T_R, float(Th[c, b]), nubar)
        print(f"{preset}: {len(far)} bins with T_R more than 1e-4 from the host's (max {float(rel.max()):.2e}), all within the "
              f"residual's rounding")
        for c in np.nonzero(fitted)[0]:
            for b in range(nb):
                if Td[c, b] > 0 and Jb[c, b] > 0:
                    B = L.rf_host_planck_integral(float(Td[c, b]), lo[b], hi[b], 0)
                    assert abs(float(Wd[c, b]) * B / Jb[c, b] - 1) <= 1.2e-7, (c, b)
        print(f"{preset}: {same} of {Td.size} bins bit-identical to the host, totals {d['totals']}")
    return d, h, est, info


@pytest.mark.parametrize("preset", ["classic", "nltenebular", "nltenebular_lineest", "ci_nltephotospheric"])
def test_fit_matches_host_build(engine_mod, preset):
    eng, model, cs, ts = _run(engine_mod, preset)
    pk_before = np.zeros(20000, dtype=abi.PACKET_DTYPE)
    eng.download_packets(pk_before)
    d, h, est, info = _compare(eng, model, cs, ts, preset)
    assert (d["flags"] & abi.RADFIELD_FITTED).all()
    # the call changes no estimator, packet or counter; a second call gives the same bits
    d2 = eng.radfield_fit(ts.c.mid, ts.c.width, synth.assocvolume_tmin(model))
    est2 = _download(eng, model, info)
    for k in ("J", "nuJ", "bfrate_raw", "radfieldbin_J", "radfieldbin_nuJ", "Jb_lu_raw", "stats", "gammaestimator"):
        assert np.array_equal(getattr(est, k), getattr(est2, k)), k
    pk_after = np.zeros(20000, dtype=abi.PACKET_DTYPE)
    eng.download_packets(pk_after)
    assert pk_before.tobytes() == pk_after.tobytes()
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, d2[k]), k
    assert d["totals"] == d2["totals"]
    # the fitted temperatures and bins feed the next step's cell state
    nxt = dict(cs.d)
    nxt.update(TR=d["TR"], TJ=d["TJ"], W=d["W"])
    if "radfieldbin_T_R" in d:
        nxt.update(radfieldbin_T_R=d["radfieldbin_T_R"].ravel(), radfieldbin_W=d["radfieldbin_W"].ravel())
    ts2 = synth.make_timestep(ts.c.start + ts.c.width, width_frac=WIDTH, vmax=model["vmax"], nts=ts.c.nts + 1)
    eng.set_cellstate(abi.CellState(nxt), ts2)
    eng.step()
    eng.close()


def test_thick_lte_seed_and_nprocs(engine_mod):
    eng, model, cs, ts = _run(engine_mod, "nltenebular", thick_below_v=0.5 * 2.4e9)
    thick = np.asarray(cs.d["thick"]) == 1
    assert 0 < thick.sum() < len(thick)
    n = model["npts_nonempty"]
    d0 = eng.radfield_fit(ts.c.mid, ts.c.width, synth.assocvolume_tmin(model))
    nbf = len(d0["bfrate_normed"]) // n
    seed = np.random.default_rng(3).uniform(1.0, 2.0, n * nbf).astype(np.float32)
    d, h, _, _ = _compare(eng, model, cs, ts, "nltenebular", seed=seed, nprocs=2)
    bf = d["bfrate_normed"].reshape(n, nbf)
    assert np.array_equal(bf[thick], seed.reshape(n, nbf)[thick])
    assert not (d["flags"][thick] & abi.RADFIELD_FITTED).any() and (d["W"][thick] == 1).all()
    assert np.array_equal(d["radfieldbin_T_R"][thick], np.asarray(cs.d["radfieldbin_T_R"], np.float32).reshape(n, -1)[thick])
    d, h, _, _ = _compare(eng, model, cs, ts, "nltenebular", lte=True, seed=seed)
    assert np.array_equal(d["bfrate_normed"], seed) and not (d["flags"] & abi.RADFIELD_FITTED).any()
    eng.close()


def test_invalid_configurations(engine_mod):
    model, cs, ts, aux = synth.build("small", ncoord=6)
    eng = engine_mod.Engine(model)
    vol = synth.assocvolume_tmin(model)
    with pytest.raises(engine_mod.EngineError, match="no cell state"):
        eng.radfield_fit(ts.c.mid, ts.c.width, vol)
    eng.set_cellstate(cs, ts)
    for kw, msg in ((dict(deltat=0.0), "deltat"), (dict(deltat=-1.0), "deltat"), (dict(nprocs=0), "nprocs"),
                    (dict(assocvolume_tmin=np.where(np.arange(len(vol)) == 3, 0.0, vol)), "assocvolume_tmin"),
                    (dict(assocvolume_tmin=-vol), "assocvolume_tmin")):
        args = dict(prev_mid=ts.c.mid, deltat=ts.c.width, assocvolume_tmin=vol)
        args.update(kw)
        with pytest.raises(engine_mod.EngineError, match=msg) as e:
            eng.radfield_fit(**args)
        assert "error -3" in str(e.value)
    d = eng.radfield_fit(ts.c.mid, ts.c.width, vol)  # and a valid call afterwards works
    assert np.isfinite(d["J"]).all()
    eng.close()
