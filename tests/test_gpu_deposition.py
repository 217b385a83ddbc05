"""The deposition rates and thickness flags on the device (artis_amd_deposition_*, artis_amd_grid_update_deposited) against the x86
build of the same rules (tests/deposition_host): per-cell arrays, flags, power vectors and totals bit for bit; the chain decay update
-> deposition update -> fit -> ion balance -> propagation against the same flags handed through the host; the refusals; and the
estimator-fed outputs before any propagation step."""
import ctypes as C

import numpy as np
import pytest

import decay_common as dc
import deposition_common as dp
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
DAY = dp.DAY
NPK = 20000
CELL_KEYS = ("eps_ana", "dep", "ntlepton_deposition_rate_density", "grey_depth", "thick")


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


@pytest.fixture(scope="module")
def nets():
    return {k: synth.decay_network(k) for k in dp.NETWORKS}


def _upload_raw(eng, raw):
    """raw [4, n] {gamma, positron, electron, alpha} into the dep_* slots of the engine's estimator block ([cell][8]: 4 gamma, 5 electron,
    6 positron, 7 alpha), everything else zero"""
    ptr, ndoubles = eng.estimators_devptr()
    n = raw.shape[1]
    block = np.zeros(ndoubles)
    rec = block[: 8 * n].reshape(n, 8)
    rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = raw[0], raw[2], raw[1], raw[3]
    eng.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert eng.L.hipMemcpy(ptr, block.ctypes.data_as(C.c_void_p), 8 * ndoubles, 1) == 0  # hipMemcpyHostToDevice


def _download_raw(eng, model):
    est = abi.Estimators(int(model["npts_nonempty"]), int(model["nbfcontinua_ground"]))
    eng.download_estimators(est)
    return np.stack([np.asarray(getattr(est, "dep_estimator_" + k), np.float64) for k in ("gamma", "positron", "electron", "alpha")])


def _state(model, cs, aux, preset, kappagrey=None):
    state = dict(cs.d)
    if preset.startswith("kilonova") and state.get("elem_meanweight") is None:
        state["elem_meanweight"] = synth.next_matter(model, cs, aux["t"], aux["t"], preset)["elem_meanweight"]
    if kappagrey is not None:
        state["kappagrey"] = kappagrey
    return abi.CellState(state)


def _setup(engine_mod, gridtype, net, preset="classic"):
    model, cs, ts, aux = dc.grid(gridtype, preset)
    n = int(model["npts_nonempty"])
    dm = synth.decay_model(model, cs, aux, net, t_model=dp.T_MODEL)
    em = synth.deposition_model(model, net)
    kappagrey = np.random.default_rng(3).uniform(0.05, 0.3, n).astype(np.float32)
    eng = engine_mod.Engine(model, preset=preset)
    eng.set_cellstate(_state(model, cs, aux, preset, kappagrey), ts)
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    return model, ts, dm, em, kappagrey, dc.HostDecay(dm, model), dp.HostDep(dm, em, model, preset), eng


def _same(got, want, keys, what):
    for k in keys:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (k, what, int((np.asarray(got[k]) != np.asarray(want[k])).sum()))


CELL_CASES = [("3d", abi.GRID_CARTESIAN3D, "medium", "classic"), ("3d", abi.GRID_CARTESIAN3D, "small_nohe4", "kilonova_lte"),
              ("1d", abi.GRID_SPHERICAL1D, "medium", "kilonova_lte"), ("1d", abi.GRID_SPHERICAL1D, "small_nohe4", "classic")]


@pytest.mark.parametrize("case", CELL_CASES, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in CELL_CASES])
def test_cells_flags_vectors_and_totals_bit_for_bit(engine_mod, nets, case):
    g, gridtype, netkind, preset = case
    model, ts, dm, em, kappagrey, hdecay, host, eng = _setup(engine_mod, gridtype, nets[netkind], preset)
    n, D = int(model["npts_nonempty"]), dp.depth()
    if g == "3d":
        assert n % 64 != 0 and n > 64
    if netkind == "medium":
        assert host.nrad > 4 * D and host.nrad % D != 0
    raw = dp.raw_estimators(n)
    _upload_raw(eng, raw)
    t_mid = dp.T_MODEL + 20.0 * DAY
    d = eng.decay_update(t_mid)
    nts, nprocs = int(ts.c.nts), 2
    first = eng.deposition_update(ts.c.mid, ts.c.width, nts, nts + 1, nts + 2, 1e30, nprocs=nprocs)
    assert (first["thick"] == abi.CELL_THIN).all()
    tau = float(np.median(first["grey_depth"]))
    out = eng.deposition_update(ts.c.mid, ts.c.width, nts, nts + 1, nts + 2, tau, nprocs=nprocs)
    assert (out["thick"] == abi.CELL_THICK).any() and (out["thick"] == abi.CELL_THIN).any()
    assert out["nradioactive"] == host.nrad and out["t_mid"] == t_mid and out["nts_next"] == nts + 1
    step = dp.step_params(model, t_mid, ts.c.mid, ts.c.width, nts + 1, nts + 2, tau, 0.0, nprocs)
    # the power vectors formed on the device from the device's coefficients are the harness's from the same coefficients
    assert out["power_vectors"].tobytes() == host.vectors(d).tobytes()
    # ... and from the device's vectors and rho the harness reproduces every array
    want = host.cells(step, out["power_vectors"], d["rho"], kappagrey, raw)
    _same(out, want, CELL_KEYS, "device vectors")
    tot, mtot = host.totmass()
    assert out["totmassnuclide"].tobytes() == tot.tobytes() and out["mtot"] == mtot
    totals = host.totals(nprocs, out["power_vectors"], raw, tot)
    assert np.array([out["totals"][k] for k in abi.DEP_TOTALS]).tobytes() == totals.tobytes()
    assert out["totals"]["gamma_dep"] > 0 and out["totals"]["eps_gamma_ana_power"] > 0 and (out["eps_ana"][0] > 0).any()
    late = eng.deposition_update(ts.c.mid, ts.c.width, nts, nts + 2, nts + 2, tau, nprocs=nprocs)  # past the grey timesteps
    assert (late["thick"] == abi.CELL_THIN).all() and late["grey_depth"].tobytes() == out["grey_depth"].tobytes()
    # the host's vectors handed in: used as they are
    Ph = host.vectors(hdecay.coeffs(t_mid))
    handed = eng.deposition_update(ts.c.mid, ts.c.width, nts, nts + 1, nts + 2, tau, nprocs=nprocs, power_vectors=Ph)
    assert handed["power_vectors"].tobytes() == Ph.tobytes()
    _same(handed, host.cells(step, Ph, d["rho"], kappagrey, raw), CELL_KEYS, "host vectors")
    assert np.array([handed["totals"][k] for k in abi.DEP_TOTALS]).tobytes() == host.totals(nprocs, Ph, raw, tot).tobytes()
    eng.close()


def test_before_any_propagation_step_the_estimator_outputs_are_zero(engine_mod, nets):
    model, ts, dm, em, kappagrey, hdecay, host, eng = _setup(engine_mod, abi.GRID_CARTESIAN3D, nets["small"], "kilonova_lte")
    eng.decay_update(ts.c.mid)
    out = eng.deposition_update(ts.c.mid, ts.c.width, int(ts.c.nts), int(ts.c.nts) + 1, 0, 1.0)
    assert (out["dep"][:4] == 0).all() and not np.signbit(out["dep"][:4]).any()  # the time-dependent build: all four from the estimators
    assert all(out["totals"][k] == 0 for k in ("gamma_dep", "positron_dep", "electron_dep", "alpha_dep"))
    assert (out["ntlepton_deposition_rate_density"] == 0).all() and (out["eps_ana"][:4] > 0).any() and out["dep"][4].tobytes() == out["eps_ana"][4].tobytes()
    eng.close()


@pytest.mark.parametrize("preset", ["classic", "kilonova_lte"])
def test_chain_on_the_device_equals_the_flags_handed_through_the_host(engine_mod, nets, preset):
    from test_gpu_decay_update import Chain

    net = nets["small"]
    ch = Chain(engine_mod, preset, net)
    ea, eb = ch.engines
    em = synth.deposition_model(ch.model, net)
    ea.deposition_setup(em)
    ts, ts_next = ch.ts, ch.ts_next
    t_mid = ts_next.c.mid
    d = ea.decay_update(t_mid)
    args = (ts.c.mid, ts.c.width, int(ts.c.nts), int(ts_next.c.nts), int(ts_next.c.nts) + 1)
    tau = float(np.median(ea.deposition_update(*args, 1e30)["grey_depth"]))
    dep = ea.deposition_update(*args, tau)
    nthick = int((dep["thick"] == abi.CELL_THICK).sum())
    assert 0 < nthick < len(dep["thick"])
    da = ea.grid_update_deposited(ts_next)
    m = eb.decay_update(t_mid)
    db = eb.grid_update_decayed(ts_next, dep["thick"])
    assert da["rho"].tobytes() == m["rho"].tobytes() == d["rho"].tobytes()
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


def test_update_matches_the_harness_on_a_steps_own_estimators(engine_mod, nets):
    """after a propagation step of 20 000 packets with gamma packets and pellets among them, the deposition update of the time-dependent
    build is the harness's from the downloaded estimators"""
    preset, net = "kilonova_lte", nets["small"]
    model, cs, ts, aux = synth.build("small", ncoord=8, options=preset, nts=10)
    dm = synth.decay_model(model, cs, aux, net, t_model=dp.T_MODEL)
    em = synth.deposition_model(model, net)
    eng = engine_mod.Engine(model, preset=preset)
    eng.set_cellstate(_state(model, cs, aux, preset), ts)
    eng.upload_packets(synth.make_packets(model, aux, NPK, kpkt_fraction=0.2, gamma_fraction=0.3, pellet_fraction=0.3))
    eng.step()
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    ts_next = synth.make_timestep(ts.c.start + ts.c.width, width_frac=0.05, vmax=model["vmax"], nts=ts.c.nts + 1)
    d = eng.decay_update(ts_next.c.mid)
    raw = _download_raw(eng, model)
    assert (raw[0] > 0).any() and (raw[1:] > 0).any()
    out = eng.deposition_update(ts.c.mid, ts.c.width, int(ts.c.nts), int(ts_next.c.nts), 0, 1.0)
    host = dp.HostDep(dm, em, model, preset)
    step = dp.step_params(model, ts_next.c.mid, ts.c.mid, ts.c.width, int(ts_next.c.nts), 0, 1.0)
    want = host.cells(step, out["power_vectors"], d["rho"], np.asarray(cs["kappagrey"], np.float32), raw)
    _same(out, want, CELL_KEYS, "the step's estimators")
    assert (out["dep"][0] > 0).any() and (out["ntlepton_deposition_rate_density"] > 0).any()
    tot, _ = host.totmass()
    assert np.array([out["totals"][k] for k in abi.DEP_TOTALS]).tobytes() == host.totals(1, out["power_vectors"], raw, tot).tobytes()
    eng.close()


def _same_download(eng, d0):
    d = eng.grid_update_download()
    for k, v in d0.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == d[k].tobytes(), k


def test_refusals_leave_the_previous_state(engine_mod, nets):
    from artis_amd.engine import EngineError
    from test_gpu_decay_update import Chain

    net = nets["small"]
    ch = Chain(engine_mod, "classic", net, nengines=1)
    ea = ch.engines[0]
    em = synth.deposition_model(ch.model, net)
    ts, ts_next = ch.ts, ch.ts_next
    t_mid = ts_next.c.mid
    nts, nts_next = int(ts.c.nts), int(ts_next.c.nts)
    fresh = engine_mod.Engine(ch.model)
    with pytest.raises(EngineError, match="error -3.*artis_amd_decay_setup"):  # no decay set-up
        fresh.deposition_setup(em)
    fresh.close()
    with pytest.raises(EngineError, match="error -3.*artis_amd_deposition_setup"):  # no deposition set-up
        ea.deposition_update(ts.c.mid, ts.c.width, nts, nts_next, 0, 1.0)
    bad = dict(em)
    bad["nuc_endecay_gamma"] = np.array(em["nuc_endecay_gamma"], copy=True)
    bad["nuc_endecay_gamma"][4] = -1.0
    with pytest.raises(EngineError, match="error -3.*nuclide 4"):
        ea.deposition_setup(bad)
    ea.deposition_setup(em)
    with pytest.raises(EngineError, match="error -3.*no decay update"):
        ea.deposition_update(ts.c.mid, ts.c.width, nts, nts_next, 0, 1.0)
    # an ordinary grid update first: its download is what every refusal below must leave
    nm = synth.next_matter(ch.model, abi.CellState(ch.state), ts.c.mid, t_mid)
    d0 = ea.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], ch.thick)
    ea.decay_update(t_mid)
    with pytest.raises(EngineError, match="error -3.*no deposition update"):
        ea.grid_update_deposited(ts_next)
    _same_download(ea, d0)
    ea.decay_update(t_mid * 1.01)
    ea.deposition_update(ts.c.mid, ts.c.width, nts, nts_next, 0, 1.0)
    with pytest.raises(EngineError, match="error -3.*another t_mid"):  # a decay update of another t_mid
        ea.grid_update_deposited(ts_next)
    _same_download(ea, d0)
    ea.decay_update(t_mid)
    with pytest.raises(EngineError, match="error -3.*not made on the decay update"):  # ... and the deposition update is still that one's
        ea.grid_update_deposited(ts_next)
    _same_download(ea, d0)
    good = ea.deposition_update(ts.c.mid, ts.c.width, nts, nts_next + 1, 0, 1.0)
    with pytest.raises(EngineError, match="error -3.*another nts"):
        ea.grid_update_deposited(ts_next)
    _same_download(ea, d0)
    ea.deposition_update(ts.c.mid, ts.c.width, nts, nts_next, 0, 1.0)
    with pytest.raises(EngineError, match="error -3.*must be NULL"):
        ea.grid_update_deposited(ts_next, _thick=ch.thick)
    _same_download(ea, d0)
    with pytest.raises(EngineError, match="error -3"):  # handed-in vectors with a power for a stable nuclide
        P = good["power_vectors"].copy()
        P[0, int(np.nonzero(net["nuc_meanlife"] <= 0)[0][0])] = 1.0
        ea.deposition_update(ts.c.mid, ts.c.width, nts, nts_next, 0, 1.0, power_vectors=P)
    assert ea.deposition_download(arrays=False)["nts_next"] == nts_next  # (the update before it stays)
    # grid_update and grid_update_decayed keep "thick is required"
    with pytest.raises(EngineError, match="error -3.*thick is required"):
        ea.grid_update_decayed(ts_next, None)
    # a new decay set-up invalidates the deposition set-up
    model, cs0, _, aux = synth.build("small", ncoord=8, options="classic", nts=10)
    ea.decay_setup(synth.decay_model(ch.model, cs0, aux, net, t_model=dp.T_MODEL))
    ea.decay_update(t_mid)
    with pytest.raises(EngineError, match="error -3.*artis_amd_deposition_setup"):
        ea.deposition_update(ts.c.mid, ts.c.width, nts, nts_next, 0, 1.0)
    ea.close()


def test_nebular_family_updates_but_does_not_hand_over(engine_mod, nets):
    from artis_amd.engine import EngineError

    net = nets["small"]
    model, cs, ts, aux = synth.build("small", ncoord=6, options="nltenebular")
    n = int(model["npts_nonempty"])
    dm = synth.decay_model(model, cs, aux, net, t_model=dp.T_MODEL)
    em = synth.deposition_model(model, net)
    eng = engine_mod.Engine(synth.with_meannucmass(model), preset="nltenebular")
    eng.set_cellstate(cs, ts)
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    raw = dp.raw_estimators(n)
    _upload_raw(eng, raw)
    d = eng.decay_update(ts.c.mid)
    nts = int(ts.c.nts)
    out = eng.deposition_update(ts.c.mid, ts.c.width, nts, nts, nts + 1, 0.0)
    host = dp.HostDep(dm, em, model, "nltenebular")
    step = dp.step_params(model, ts.c.mid, ts.c.mid, ts.c.width, nts, nts + 1, 0.0)
    _same(out, host.cells(step, out["power_vectors"], d["rho"], np.asarray(cs["kappagrey"], np.float32), raw), CELL_KEYS, "nltenebular")
    assert out["power_vectors"].tobytes() == host.vectors(d).tobytes()
    with pytest.raises(EngineError, match="error -4"):
        eng.grid_update_deposited(ts)
    eng.close()
