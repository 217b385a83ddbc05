"""The decay and abundance update on the device (artis_amd_decay_*, artis_amd_grid_update_decayed) against the x86 build of the same
rules (tests/decay_host): the coefficients to the Bateman sum's rounding bound (the two machines differ in exp's last bits), the
per-cell kernels bit for bit, the chain decay update -> ion balance -> propagation against the same matter handed through the host,
and the refusals."""
import numpy as np
import pytest

import decay_common as dc
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
DAY, EPS = dc.DAY, dc.EPS
WIDTH = 0.05
NPK = 20000


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


@pytest.fixture(scope="module")
def nets():
    return {k: synth.decay_network(k) for k in ("small", "small_nohe4")}


def _setup(engine_mod, gridtype, net, preset="classic"):
    model, cs, ts, aux = dc.grid(gridtype, preset)
    dm = synth.decay_model(model, cs, aux, net, t_model=dc.T_MODEL)
    eng = engine_mod.Engine(model, preset=preset)
    eng.decay_setup(dm)
    return model, dm, dc.HostDecay(dm, model), eng


def _ulps64(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def test_device_coefficients_within_the_rounding_bound_of_the_host(engine_mod, nets):
    """Per path |device - x86| of the Bateman sum <= 4 (L + x_dom) 2^-52 scale (the cap of tests/test_decay_update_rules.py, far
    looser than what exp's last bits move), carried to the coefficients by their exact factors branchproduct x A_end / A_top (He4:
    x 4 / A_top, with the scale of the sum whose last decay constant is zeroed); surviving fractions within 2 ulp."""
    net = nets["small"]
    model, dm, host, eng = _setup(engine_mod, abi.GRID_SPHERICAL1D, net)
    A = net["nuc_a"].astype(np.float64)
    L = np.diff(net["path_start"]).astype(np.float64)
    top = net["path_nucindex"][net["path_start"][:-1]]
    end = net["path_nucindex"][net["path_start"][1:] - 1]
    alpha = np.nonzero(net["path_last_decaytype"] == abi.DECAYTYPE_ALPHA)[0]
    worst, one_sided = 0.0, 0
    for days in dc.TIMES_DAYS:
        t_mid = dc.T_MODEL + days * DAY
        d = eng.decay_update(t_mid)
        h = host.coeffs(t_mid)
        assert np.allclose(d["path_scale"], h["path_scale"], rtol=1e-12, atol=0)
        bar = 4 * (L + h["path_x_dom"]) * EPS * h["path_scale"] * net["path_branchproduct"] * A[end] / A[top]
        diff = np.abs(d["endnuc_coeff"] - h["endnuc_coeff"])
        assert (diff <= bar).all(), (days, int(np.argmax(diff - bar)))
        worst = max(worst, float(np.max(diff[bar > 0] / bar[bar > 0], initial=0.0)))
        one_sided += int(((d["endnuc_coeff"] == 0) != (h["endnuc_coeff"] == 0)).sum())
        for p in alpha:
            lam = dc.path_lambdas(net, p)
            _, scale, x = dc.decaychain(np.concatenate([lam[:-1], [0.0]]), days * DAY)
            b = 4 * (L[p] + x) * EPS * scale * net["path_branchproduct"][p] * 4.0 / A[top[p]]
            dh = abs(d["he4_coeff"][p] - h["he4_coeff"][p])
            assert dh <= b, (days, p)
            worst = max(worst, dh / b if b > 0 else 0.0)
            one_sided += int((d["he4_coeff"][p] == 0) != (h["he4_coeff"][p] == 0))
        assert (np.delete(d["he4_coeff"], alpha) == 0).all()
        assert _ulps64(d["survivingfrac"], h["survivingfrac"]).max() <= 2
        if days == 0.0:
            assert (d["endnuc_coeff"] == 0).all() and (d["he4_coeff"] == 0).all() and (d["survivingfrac"] == 1).all()
    print(f"worst |device - x86| / bar = {worst:.4f}; {one_sided} coefficients clamped to 0 on one side only")
    eng.close()


CELL_CASES = [("3d", abi.GRID_CARTESIAN3D, "small", "classic"), ("3d", abi.GRID_CARTESIAN3D, "small_nohe4", "kilonova_lte"),
              ("1d", abi.GRID_SPHERICAL1D, "small", "kilonova_lte"), ("1d", abi.GRID_SPHERICAL1D, "small_nohe4", "classic")]


@pytest.mark.parametrize("case", CELL_CASES, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in CELL_CASES])
def test_cell_kernels_bit_for_bit(engine_mod, nets, case):
    _, gridtype, netkind, preset = case
    model, dm, host, eng = _setup(engine_mod, gridtype, nets[netkind], preset)
    keys = ("rho", "elem_massfracs", "elem_meanweight")
    for days in (20.0, 300.0):
        t_mid = dc.T_MODEL + days * DAY
        co = host.coeffs(t_mid)
        want = host.cells(t_mid, co)
        for nuclides in (True, False):
            # the host's coefficients handed in: every array is the harness's
            d = eng.decay_update(t_mid, coeffs=co, want_nuclides=nuclides)
            for k in ("endnuc_coeff", "he4_coeff", "survivingfrac"):
                assert d[k].tobytes() == co[k].tobytes(), k
            for k in keys + (("nuc_massfracs",) if nuclides else ()):
                assert d[k].tobytes() == want[k].tobytes(), (k, days, nuclides, int((d[k] != want[k]).sum()))
            assert ("nuc_massfracs" in d) == nuclides and d["t_mid"] == t_mid and d["he4_nucindex"] == host.he4
            # the device's own coefficients: the harness reproduces every array from them
            d = eng.decay_update(t_mid, want_nuclides=nuclides)
            again = host.cells(t_mid, d)
            for k in keys + (("nuc_massfracs",) if nuclides else ()):
                assert d[k].tobytes() == again[k].tobytes(), (k, days, nuclides, "device coefficients")
    assert d["rho"].min() > 0 and np.isfinite(d["elem_meanweight"]).all() and (d["elem_meanweight"] > 0).all()
    eng.close()


class Chain:
    """engines in one state after a propagation step and a radiation-field fit of the same estimators, each with the decay network"""

    def __init__(self, engine_mod, preset, net, nengines=2):
        model, cs0, ts, aux = synth.build("small", ncoord=8, options=preset, nts=10)
        if not preset.startswith("kilonova"):
            model = synth.with_meannucmass(model)
        self.model, self.preset, self.ts = model, preset, ts
        state = dict(cs0.d)
        if preset.startswith("kilonova") and state.get("elem_meanweight") is None:
            state["elem_meanweight"] = synth.next_matter(model, cs0, aux["t"], aux["t"], preset)["elem_meanweight"]
        self.state, self.thick = state, np.asarray(state["thick"], np.int32)
        pk0 = synth.make_packets(model, aux, NPK, kpkt_fraction=0.2, ts_width_frac=(1.0 + WIDTH) ** 4 - 1.0)
        dm = synth.decay_model(model, cs0, aux, net, t_model=dc.T_MODEL)
        vol = synth.assocvolume_tmin(model)
        self.engines = []
        for _ in range(nengines):
            eng = engine_mod.Engine(model, preset=preset)
            eng.set_cellstate(abi.CellState(state), ts)
            eng.upload_packets(pk0)
            eng.step()
            eng.decay_setup(dm)
            self.engines.append(eng)
        # the estimators are sums of device-wide atomics whose last bits differ from run to run: every engine fits the first one's block
        import ctypes as C

        hip = self.engines[0].L
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        src, ndoubles = self.engines[0].estimators_devptr()
        for eng in self.engines[1:]:
            dst, nd = eng.estimators_devptr()
            assert nd == ndoubles and hip.hipMemcpy(dst, src, 8 * ndoubles, 3) == 0  # hipMemcpyDeviceToDevice
        for eng in self.engines:
            eng.radfield_fit(ts.c.mid, ts.c.width, vol)
        self.ts_next = synth.make_timestep(ts.c.start + ts.c.width, width_frac=WIDTH, vmax=model["vmax"], nts=ts.c.nts + 1)


@pytest.mark.parametrize("preset", ["classic", "kilonova_lte"])
def test_chain_on_the_device_equals_the_matter_handed_through_the_host(engine_mod, nets, preset):
    ch = Chain(engine_mod, preset, nets["small"])
    ea, eb = ch.engines
    t_mid = ch.ts_next.c.mid
    ea.decay_update(t_mid)
    da = ea.grid_update_decayed(ch.ts_next, ch.thick)
    m = eb.decay_update(t_mid)
    db = eb.grid_update(ch.ts_next, m["rho"], m["elem_massfracs"], ch.thick,
                        elem_meanweight=m["elem_meanweight"] if preset.startswith("kilonova") else None)
    assert da["rho"].tobytes() == m["rho"].tobytes()
    for k, v in da.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == db[k].tobytes(), k
    assert da["ncells_flagged"] == db["ncells_flagged"] and da["total_evals"] == db["total_evals"]
    # one propagation step from the two states
    n, g = int(ch.model["npts_nonempty"]), int(ch.model["nbfcontinua_ground"])
    outs = []
    for eng in (ea, eb):
        eng.zero_estimators()
        eng.step()
        p = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
        eng.download_packets(p)
        est = abi.Estimators(n, g)
        eng.download_estimators(est)
        outs.append((p, est))
    (pa, sa), (pb, sb) = outs
    assert pa.tobytes() == pb.tobytes()  # generator states included
    assert np.array_equal(sa.stats, sb.stats)
    # the estimators are sums of device-wide f64 atomics, whose order differs from run to run: the bar of
    # tests/test_gpu_estimator_paths.py between two runs of the same packets
    for k in ("J", "nuJ", "ffheatingestimator", "colheatingestimator", "gammaestimator", "bfheatingestimator"):
        a, b = np.asarray(getattr(sa, k)), np.asarray(getattr(sb, k))
        assert np.array_equal(a == 0, b == 0), k
        assert np.all(np.abs(a - b) <= 1e-12 * np.abs(a)), k
    ea.close()
    eb.close()


def _same_download(eng, d0):
    d = eng.grid_update_download()
    for k, v in d0.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == d[k].tobytes(), k


def test_refusals_leave_the_cell_state(engine_mod, nets):
    from artis_amd.engine import EngineError

    ch = Chain(engine_mod, "classic", nets["small"], nengines=1)
    ea = ch.engines[0]
    fresh = engine_mod.Engine(ch.model)
    with pytest.raises(EngineError, match="error -3.*artis_amd_decay_setup"):
        fresh.decay_update(ch.ts_next.c.mid)
    fresh.close()
    with pytest.raises(EngineError, match="error -3"):  # before t_model
        ea.decay_update(0.5 * dc.T_MODEL)
    # an ordinary grid update first: its download is what every refusal below must leave
    nm = synth.next_matter(ch.model, abi.CellState(ch.state), ch.ts.c.mid, ch.ts_next.c.mid)
    d0 = ea.grid_update(ch.ts_next, nm["rho"], nm["elem_massfracs"], ch.thick)
    with pytest.raises(EngineError, match="error -3.*no decay update"):
        ea.grid_update_decayed(ch.ts_next, ch.thick)
    _same_download(ea, d0)
    ea.decay_update(ch.ts_next.c.mid * 1.01)
    with pytest.raises(EngineError, match="error -3.*another t_mid"):
        ea.grid_update_decayed(ch.ts_next, ch.thick)
    _same_download(ea, d0)
    m = ea.decay_update(ch.ts_next.c.mid)
    with pytest.raises(EngineError, match="error -3.*must be NULL"):
        ea.grid_update_decayed(ch.ts_next, ch.thick, _matter=(m["rho"], m["elem_massfracs"], None))
    _same_download(ea, d0)
    ea.close()


def test_nebular_family_updates_but_does_not_hand_over(engine_mod, nets):
    from artis_amd.engine import EngineError

    model, cs, ts, aux = synth.build("small", ncoord=6, options="nltenebular")
    dm = synth.decay_model(model, cs, aux, nets["small"], t_model=dc.T_MODEL)
    eng = engine_mod.Engine(synth.with_meannucmass(model), preset="nltenebular")
    eng.set_cellstate(cs, ts)
    eng.decay_setup(dm)
    d = eng.decay_update(ts.c.mid, want_nuclides=True)
    again = dc.HostDecay(dm, model).cells(ts.c.mid, d)
    for k in ("rho", "elem_massfracs", "elem_meanweight", "nuc_massfracs"):
        assert d[k].tobytes() == again[k].tobytes(), k
    with pytest.raises(EngineError, match="error -4"):
        eng.grid_update_decayed(ts, cs["thick"])
    eng.close()
