"""The thermal balance of the thin cells on the device (artis_amd_thermal_*, artis_amd_grid_update_thermal) against the x86 build of the
same rules (tests/thermal_host) applied to the downloaded estimators, fit and cell state, on the synthetic models (classic 3D with a
thick core, classic 1D). The renormalisation is arithmetic only and must be bit-equal. Gamma, and phi and the rates of the final
evaluation -- the x86 rules evaluated at the device's own T_e, Gamma and partition functions -- are held to 1e-13, the bar for the
device's exp / pow against glibc's in positive sums (tests/test_gpu_ion_balance.py; Gamma and U use them, the rates the stage's own). Two machines may bracket the root with different
last bits, so T_e is held to 2 x TEMPERATURE_SOLVER_ACCURACY: both brackets are at most one accuracy wide and
tests/test_thermal_balance_rules.py shows that the root they hold is unique (the factor 2: the precedent of the n_e bar, 2e-3 for 1e-3).
The state the hand-over leaves must propagate packets exactly as the same arrays handed over through artis_amd_set_cellstate.
Two comparisons are narrower than "the solve against the harness's own solve", on purpose: phi and the rates are those of the final
evaluation, which the two machines make at their own T_e, so they are compared with the x86 rules evaluated at the DEVICE's T_e, Gamma
and U, and directly with the harness's solve in the cells whose stored T_e is the same float; and the two damping flags are left out of
the flag comparison, because a solution within the T_e bar of 2 x or 0.5 x the old T_e may fall on either side of it."""
import ctypes as C

import numpy as np
import pytest

import thermal_common as tc
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
NPK = 20000
CASES = [dict(id="classic_3d_thick_core", gridtype=abi.GRID_CARTESIAN3D), dict(id="classic_1d", gridtype=abi.GRID_SPHERICAL1D)]
HEATING = ("ntlepton_dep", "dep_alpha", "dep_spfission")


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - b) / np.abs(b)
    return np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0.0, r)


class Run:
    """one model, its packets and a host mirror of the cell state"""

    def __init__(self, gridtype=abi.GRID_CARTESIAN3D, thick_below_v=1e9):
        self.model, cs0, _, aux = tc.build_model(gridtype, thick_below_v)
        self.pk0 = synth.make_packets(self.model, aux, NPK, kpkt_fraction=0.2, ts_width_frac=(1.0 + tc.WIDTH) ** 4 - 1.0)
        self.state = dict(cs0.d)
        self.ts = synth.make_timestep(aux["t"], width_frac=tc.WIDTH, vmax=self.model["vmax"], nts=10)
        self.ts_next = tc.next_timestep(self.model, self.ts)
        self.nm = synth.next_matter(self.model, abi.CellState(self.state), self.ts.c.mid, self.ts_next.c.mid, "classic")
        self.hm = tc.HostModel(self.model)
        self.vol = synth.assocvolume_tmin(self.model)

    def engine(self, engine_mod, preset="classic"):
        eng = engine_mod.Engine(self.model, preset=preset)
        eng.set_cellstate(abi.CellState(self.state), self.ts)
        eng._npk = NPK
        return eng

    def step_and_fit(self, eng):
        eng.upload_packets(self.pk0)
        eng.step()
        return eng.radfield_fit(self.ts.c.mid, self.ts.c.width, self.vol, lte_iteration=False)

    def inputs(self, eng, fit):
        """the x86 rules' inputs from the engine's estimators and fit, with the synthetic heating inputs made for them"""
        n, g = self.hm.n, self.hm.g
        est = abi.Estimators(n, g)
        eng.download_estimators(est)
        ins = tc.call_inputs(self.model, self.state, self.ts, self.nm, fit, np.asarray(est.gammaestimator).reshape(n, g).copy(),
                             np.asarray(est.ffheatingestimator).copy(), np.asarray(est.colheatingestimator).copy(), self.vol)
        ins.update(tc.heating_inputs(self.hm, ins))
        return ins

    def solve(self, eng, ins):
        return eng.thermal_solve(ins["bfheat"], rho=self.nm["rho"], elem_massfracs=self.nm["elem_massfracs"], **{k: ins[k] for k in HEATING})

    def handover_state(self, d, t):
        """the arrays grid_update_thermal wrote into the engine's cell state, as a host would hand them over through set_cellstate"""
        s = dict(self.state)
        for k in ("Te", "TJ", "TR", "W", "nne", "nnetot", "rho"):
            s[k] = d[k]
        s["ion_partfuncts"] = d["ion_partfuncts"].ravel()
        s["ion_groundlevelpops"] = d["ion_groundlevelpops"].ravel()
        s["elem_massfracs"] = self.nm["elem_massfracs"]
        s["thick"] = self.nm["thick"]
        forced = (d["flags"] & abi.IONBAL_FORCED_SAHA) != 0
        renorm = t["corrphotoionrenorm"].copy()
        renorm[forced] = 1.0
        s["corrphotoionrenorm"] = renorm.ravel()
        return s


def _step_and_compare(ea, eb, model, label):
    """one step of both engines from the same packets and zeroed estimators: packets, counters and estimators identical
    (tests/test_gpu_ion_balance.py's checks)"""
    n, g = int(model["npts_nonempty"]), int(model["nbfcontinua_ground"])
    outs = []
    for eng in (ea, eb):
        eng.zero_estimators()
        eng.step()
    for eng in (ea, eb):
        p = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
        eng.download_packets(p)
        est = abi.Estimators(n, g)
        eng.download_estimators(est)
        outs.append((p, est))
    (pa, sa), (pb, sb) = outs
    assert pa.tobytes() == pb.tobytes(), label
    assert np.array_equal(sa.stats, sb.stats), label
    # the estimators are sums of device-wide f64 atomics, whose order differs from run to run: the bar of
    # tests/test_gpu_estimator_paths.py between two runs of the same packets
    for k in ("J", "nuJ", "ffheatingestimator", "colheatingestimator", "gammaestimator", "bfheatingestimator"):
        a, b = np.asarray(getattr(sa, k)), np.asarray(getattr(sb, k))
        assert np.array_equal(a == 0, b == 0), (label, k)
        assert np.all(np.abs(a - b) <= 1e-12 * np.abs(a)), (label, k, float(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-300))))


@pytest.fixture(scope="module", params=CASES, ids=[c["id"] for c in CASES])
def solved(engine_mod, request):
    """one step, fit and solve of a case on the device, and the x86 rules on the downloaded inputs (shared by the tests below)"""
    case = request.param
    run = Run(case["gridtype"])
    eng = run.engine(engine_mod)
    fit = run.step_and_fit(eng)
    ins = run.inputs(eng, fit)
    h = run.hm.solve(ins)
    d = run.solve(eng, ins)
    eng.close()
    fitted = (fit["flags"] & abi.RADFIELD_FITTED) != 0
    uU = _ulps(d["ion_partfuncts"], h["U"])
    bit_equal = (uU == 0).all(axis=1) & (d["phi"] == h["phi"]).all(axis=1) & (d["gamma"] == h["gamma"]).all(axis=1) & (d["evals"] == h["evals"])
    return dict(case=case, run=run, fit=fit, ins=ins, h=h, d=d, fitted=fitted, uU=uU, bit_equal=bit_equal & fitted)


OUTPUT_PAIRS = (("Te", "Te"), ("Te_solved", "Te_solved"), ("bracket", "bracket"), ("flags", "flags"), ("evals", "evals"), ("nne", "nne"),
                ("ion_groundlevelpops", "ground"), ("phi", "phi"), ("rates", "rates"))


def test_solve_matches_host_rules(solved):
    case, run, fit, ins, h, d, fitted, uU = (solved[k] for k in ("case", "run", "fit", "ins", "h", "d", "fitted", "uU"))
    hm = run.hm
    label = case["id"]
    n = hm.n
    assert d["nfitted"] == fitted.sum() and 0 < d["nfitted"] <= n
    if case["gridtype"] == abi.GRID_CARTESIAN3D:
        assert d["nfitted"] < n  # (the thick core)
    # the renormalisation: arithmetic only
    assert np.array_equal(d["corrphotoionrenorm"], h["renorm"]), label
    # unfitted cells: untouched
    assert np.array_equal(d["Te"][~fitted], fit["Te"][~fitted]) and not d["flags"][~fitted].any() and not d["evals"][~fitted].any()
    worst_gamma = float(_rel(d["gamma"], h["gamma"]).max(initial=0))
    # the final evaluation: the x86 rules at the device's own T_e, Gamma and partition functions
    at_dev = dict(_raw=dict(U=d["ion_partfuncts"].ravel(), gamma=np.resize(d["gamma"].ravel(), h["_raw"]["gamma"].shape)))
    hr = hm.rates(ins, Te=d["Te"], rebalance=True, solved=at_dev)
    worst_phi = float(_rel(d["phi"][fitted], hr["phi"][fitted]).max(initial=0))
    worst_rate = float(_rel(d["rates"][fitted], hr["rates"][fitted])[:, :8].max(initial=0))
    res_scale = np.abs(hr["rates"][fitted][:, :8]).sum(axis=1)  # (heating - cooling cancels: held to the terms it is formed from)
    worst_res = float((np.abs(d["rates"][fitted][:, 8] - hr["rates"][fitted][:, 8]) / res_scale).max(initial=0))
    same_state = np.array_equal(d["nne"][fitted], hr["nne"][fitted]) and np.array_equal(d["ion_groundlevelpops"][fitted], hr["ground"][fitted])
    print(f"{label}: worst relative difference Gamma {worst_gamma:.3e}, phi {worst_phi:.3e}, rates {worst_rate:.3e}, residual {worst_res:.3e}; "
          f"U entries one ulp apart {int((uU == 1).sum())}, more {int((uU > 1).sum())}; n_e and populations at the device's T_e identical: {same_state}")
    # T_e between the two machines
    bd, bh = (d["flags"] & abi.THERMAL_BRACKETED) != 0, (h["flags"] & abi.THERMAL_BRACKETED) != 0
    both = bd & bh
    rel_T = np.abs(d["Te_solved"][both] / h["Te_solved"][both] - 1)
    print(f"{label}: {int(bd.sum())} bracketed cells of {int(fitted.sum())} fitted, worst T_e difference {float(rel_T.max(initial=0)):.3e} "
          f"(bar {2 * hm.accuracy:g}); cells with U, phi, Gamma and evaluation count bit-equal: {int(solved['bit_equal'].sum())} of {int(fitted.sum())}; "
          f"flags {d['ncells_flagged']}, {d['total_evals']} evaluations, kernel ms {d['kernel_ms']}")
    assert uU.max(initial=0) <= 1, label
    assert worst_gamma <= 1e-13, label
    assert worst_phi <= 1e-13 and worst_rate <= 1e-13 and worst_res <= 1e-13, label
    assert np.array_equal(d["rates"][fitted][:, 9], hr["rates"][fitted][:, 9])  # dep_frac_heating: arithmetic only
    assert np.array_equal(bd, bh), label
    assert rel_T.max(initial=0) <= 2 * hm.accuracy, label
    thermal_bits = 0xFF00 & ~(abi.THERMAL_DAMPED_UP | abi.THERMAL_DAMPED_DOWN)  # (a solution at 2 x or 0.5 x the old T_e may fall either way)
    assert np.array_equal(d["flags"] & thermal_bits, h["flags"] & thermal_bits), label
    # every bracketed cell of the device holds the finder's certificate, by the x86 residual at the device's bracket
    tc.certificate(hm, ins, h, d, np.nonzero(bd)[0])
    # directly against the harness's own solve where both machines stored the same T_e (and formed the same U)
    same_Te = fitted & (d["Te"] == h["Te"]) & (uU == 0).all(axis=1)
    assert same_Te.sum() * 2 >= fitted.sum(), (label, int(same_Te.sum()))
    assert float(_rel(d["phi"][same_Te], h["phi"][same_Te]).max(initial=0)) <= 1e-13, label
    assert float(_rel(d["rates"][same_Te][:, :8], h["rates"][same_Te][:, :8]).max(initial=0)) <= 1e-13, label
    assert solved["bit_equal"].sum() * 2 >= fitted.sum(), (label, int(solved["bit_equal"].sum()))
    # a cell whose U and Gamma are bit-equal takes the same path on both machines (the stage's own exp and log): the counts agree
    same_in = (uU == 0).all(axis=1) & (d["gamma"] == h["gamma"]).all(axis=1) & fitted
    assert np.array_equal(d["evals"][same_in], h["evals"][same_in]), label


def test_bit_equal_cells_have_every_output_bit_equal(solved):
    """A cell whose U, phi and Gamma are bit-equal and whose evaluation count matches has EVERY output bit-equal: the rates of a trial
    state are formed with the stage's own exp and log (thermal_balance.h tb_exp, tb_log), plain IEEE arithmetic in one order on both
    machines, so the search reads the same residuals and takes the same steps. The figures are printed before the assertion."""
    d, h, sel, label = solved["d"], solved["h"], solved["bit_equal"], solved["case"]["id"]
    for k_d, k_h in OUTPUT_PAIRS:
        a, b = d[k_d][sel], h[k_h][sel]
        same = np.array([np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)])
        worst = float(_rel(a, b).max(initial=0)) if a.dtype.kind == "f" else 0.0
        print(f"{label}: {k_d}: bit-equal in {int(same.sum())} of {int(sel.sum())} selected cells, worst relative difference {worst:.3e}")
    for k_d, k_h in OUTPUT_PAIRS:
        assert np.array_equal(d[k_d][sel], h[k_h][sel], equal_nan=True), (label, k_d)


def test_handover_matches_set_cellstate(engine_mod):
    run = Run()
    ea, eb = run.engine(engine_mod), run.engine(engine_mod)
    fit = run.step_and_fit(ea)
    ins = run.inputs(ea, fit)
    t = run.solve(ea, ins)
    # (a rates call at other temperatures in between writes the result block, not what the hand-over takes)
    ea.thermal_rates(ins["bfheat"], Te=t["Te"] * np.float32(1.1), rebalance=True, **{k: ins[k] for k in HEATING})
    d = ea.grid_update_thermal(run.ts_next, thick=run.nm["thick"])
    fitted = (fit["flags"] & abi.RADFIELD_FITTED) != 0
    # the balance ran at the solve's T_e with its Gamma: the populations are those of the solve's final evaluation
    assert np.array_equal(d["Te"], t["Te"])
    assert np.array_equal(d["gamma_normed"][fitted], t["gamma"][fitted])
    assert np.array_equal(d["ion_partfuncts"][fitted], t["ion_partfuncts"][fitted])
    assert np.array_equal(d["ion_groundlevelpops"][fitted], t["ion_groundlevelpops"][fitted]) and np.array_equal(d["nne"][fitted], t["nne"][fitted])
    assert np.array_equal((d["flags"] & abi.IONBAL_FORCED_SAHA) != 0, ~fitted)
    pk = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
    ea.download_packets(pk)
    eb.set_cellstate(abi.CellState(run.handover_state(d, t)), run.ts_next)
    eb.upload_packets(pk)
    _step_and_compare(ea, eb, run.model, "handover")
    ea.close()
    eb.close()


def test_rates_match_host_rules_and_the_solve(engine_mod):
    """thermal_rates without the ion balance (the resident state at the resident T_e) against the x86 rules in every cell, to the bar
    of the device's exp / pow in positive sums; with it, at the solve's T_e, the solve's own final evaluation bit for bit"""
    run = Run()
    hm = run.hm
    eng = run.engine(engine_mod)
    fit = run.step_and_fit(eng)
    ins = run.inputs(eng, fit)
    heat = {k: ins[k] for k in HEATING}
    d0 = eng.thermal_rates(ins["bfheat"], Te=None, rebalance=False, **heat)
    resident = dict(ins, rho=run.state["rho"], massfrac=run.state["elem_massfracs"])
    h0 = hm.rates(resident, Te=None, rebalance=False)
    worst = float(_rel(d0["rates"][:, :8], h0["rates"][:, :8]).max(initial=0))
    print(f"rates of the resident state: worst relative difference {worst:.3e} over {hm.n} cells, kernel ms {d0['kernel_ms']['rates']:.3f}")
    assert worst <= 1e-13 and (h0["rates"][:, :3] > 0).all()
    assert np.array_equal(d0["Te"], np.asarray(run.state["Te"], np.float32)) and np.array_equal(d0["nne"], np.asarray(run.state["nne"], np.float32))
    with pytest.raises(engine_mod.EngineError, match="error -3"):  # rebalance = 1 before any solve
        eng.thermal_rates(ins["bfheat"], Te=None, rebalance=True, **heat)
    t = run.solve(eng, ins)
    d1 = eng.thermal_rates(ins["bfheat"], Te=t["Te"], rebalance=True, **heat)
    eng.close()
    fitted = (fit["flags"] & abi.RADFIELD_FITTED) != 0
    for k in ("rates", "nne", "ion_groundlevelpops", "phi", "Te"):
        assert d1[k][fitted].tobytes() == t[k][fitted].tobytes(), k


def test_device_to_device_call_order(engine_mod):
    """the documented call order: matter NULL (the decay update's arrays), deposition inputs NULL (the deposition update's block), thick
    NULL (its flags). The solve gives the bytes of the same solve fed the downloads of those stages as host arrays, and the state the
    hand-over leaves propagates packets as the same arrays handed over through set_cellstate, thick included."""
    import deposition_common as dp

    run = Run()
    net = synth.decay_network("small")
    model, cs0, _, aux = tc.build_model()
    ea, eb = run.engine(engine_mod), run.engine(engine_mod)
    ea.upload_packets(run.pk0)
    ea.step()
    ea.decay_setup(synth.decay_model(model, cs0, aux, net, t_model=dp.T_MODEL))
    ea.deposition_setup(synth.deposition_model(model, net))
    dec = ea.decay_update(run.ts_next.c.mid)
    nts = int(run.ts.c.nts)
    tau = float(np.median(ea.deposition_update(run.ts.c.mid, run.ts.c.width, nts, nts + 1, nts + 2, 1e30)["grey_depth"]))
    dep = ea.deposition_update(run.ts.c.mid, run.ts.c.width, nts, nts + 1, nts + 2, tau)
    assert 0 < (dep["thick"] == tc.CELL_THICK).sum() < run.hm.n
    fit = ea.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol, lte_iteration=False)
    bfheat = np.full((run.hm.n, run.hm.nl), 1e-20)
    t_dev = ea.thermal_solve(bfheat)
    t_host = ea.thermal_solve(bfheat, rho=dec["rho"], elem_massfracs=dec["elem_massfracs"], ntlepton_dep=dep["ntlepton_deposition_rate_density"],
                              dep_alpha=dep["dep"][3], dep_spfission=dep["dep"][4])
    for k, v in t_dev.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == t_host[k].tobytes(), k
    assert (t_dev["flags"] & (abi.THERMAL_BRACKETED | abi.THERMAL_PINNED_LOW | abi.THERMAL_PINNED_HIGH)).any()
    assert (t_dev["rates"][:, 7] > 0).any()  # (heating_dep from the device's block)
    d = ea.grid_update_thermal(run.ts_next)
    assert np.array_equal(d["rho"], dec["rho"]) and np.array_equal(d["Te"], t_dev["Te"])
    pk = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
    ea.download_packets(pk)
    run.nm = dict(run.nm, elem_massfracs=dec["elem_massfracs"].ravel(), thick=dep["thick"])
    eb.set_cellstate(abi.CellState(run.handover_state(d, t_dev)), run.ts_next)
    eb.upload_packets(pk)
    _step_and_compare(ea, eb, run.model, "device to device")
    ea.close()
    eb.close()


def test_two_calls_identical(engine_mod):
    run = Run()
    eng = run.engine(engine_mod)
    fit = run.step_and_fit(eng)
    ins = run.inputs(eng, fit)
    a, b = run.solve(eng, ins), run.solve(eng, ins)
    eng.close()
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == b[k].tobytes(), k
    assert a["ncells_flagged"] == b["ncells_flagged"] and a["total_evals"] == b["total_evals"]


def test_tiled_cache_engine_gives_the_same_download(engine_mod, monkeypatch):
    """the stage reads the cell state, the estimators and the fit, never the cell cache: an engine whose cache holds a third of the
    rows at a time gives the same bytes from the same estimators (B's block is overwritten with A's, device to device: the sums of two
    runs' atomics differ in their last bits)"""
    run = Run()
    ea = run.engine(engine_mod)
    _, _, bpc = ea.cache_tiles()
    monkeypatch.setenv("ARTIS_AMD_MA_HOTFRAC", "1")
    monkeypatch.setenv("ARTIS_AMD_MA_POOLFRAC", "1")
    monkeypatch.setenv("ARTIS_AMD_CACHE_BUDGET_MB", f"{bpc * run.hm.n / 3 / 2**20:.3f}")
    eb = run.engine(engine_mod)
    assert ea.cache_tiles()[0] == 1 and eb.cache_tiles()[0] > 1
    for eng in (ea, eb):
        eng.upload_packets(run.pk0)
        eng.step()
    (pa, na), (pb, nb) = ea.estimators_devptr(), eb.estimators_devptr()
    assert na == nb
    import torch  # (the HIP runtime the process already has)

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    assert hip.hipMemcpy(pb, pa, 8 * na, 3) == 0  # hipMemcpyDeviceToDevice
    outs = []
    for eng in (ea, eb):
        fit = eng.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol, lte_iteration=False)
        if not outs:
            ins = run.inputs(eng, fit)
        outs.append(run.solve(eng, ins))
        eng.close()
    for k, v in outs[0].items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == outs[1][k].tobytes(), k


def test_refusals(engine_mod):
    from artis_amd.engine import EngineError

    run = Run()
    eng = run.engine(engine_mod)
    eng.upload_packets(run.pk0)
    eng.step()
    bfheat = np.zeros((run.hm.n, run.hm.nl))
    zeros = {k: np.zeros(run.hm.n) for k in HEATING}
    with pytest.raises(EngineError, match="error -3"):  # no fit since the last step
        eng.thermal_solve(bfheat, rho=run.nm["rho"], elem_massfracs=run.nm["elem_massfracs"], **zeros)
    eng.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol)
    with pytest.raises(EngineError, match="error -3"):  # no bfheatingcoeffs
        eng.thermal_solve(None, rho=run.nm["rho"], elem_massfracs=run.nm["elem_massfracs"], **zeros)
    with pytest.raises(EngineError, match="error -3"):  # no solve yet
        eng.grid_update_thermal(run.ts_next, thick=run.nm["thick"])
    eng.thermal_solve(bfheat, rho=run.nm["rho"], elem_massfracs=run.nm["elem_massfracs"], **zeros)
    with pytest.raises(EngineError, match="error -3"):  # host matter handed to grid_update_thermal
        u, keep = abi.grid_update_config(True, run.nm["rho"], run.nm["elem_massfracs"], run.nm["thick"])
        eng._check(eng.L.artis_amd_grid_update_thermal(eng.h, C.byref(u), C.cast(run.ts_next.ref(), C.c_void_p), None))
    with pytest.raises(EngineError, match="error -3"):  # a clumpfactor handed to the hand-over (it takes the solve's)
        u, keep = abi.grid_update_config(True, None, None, run.nm["thick"], clumpfactor=run.state["clumpfactor"])
        eng._check(eng.L.artis_amd_grid_update_thermal(eng.h, C.byref(u), C.cast(run.ts_next.ref(), C.c_void_p), None))
    eng.set_cellstate(abi.CellState(run.state), run.ts)
    with pytest.raises(EngineError, match="error -3"):  # a cell state set since the solve
        eng.grid_update_thermal(run.ts_next, thick=run.nm["thick"])
    with pytest.raises(EngineError, match="error -3"):
        eng.thermal_rates(bfheat, rebalance=True, **zeros)
    eng.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol)
    with pytest.raises(EngineError, match="error -3"):  # a fit newer than the solve
        eng.grid_update_thermal(run.ts_next, thick=run.nm["thick"])
    eng.close()
    # builds the stage is not written for: the text names the option
    for preset, option in (("nltenebular", "LTEPOP_EXCITATION_USE_TJ"), ("kilonova_lte", "DIRECT_COL_HEAT")):
        model, cs, ts, aux = synth.build("small", ncoord=6, options=preset)
        e2 = engine_mod.Engine(synth.with_meannucmass(model), preset=preset)
        e2.set_cellstate(cs, ts)
        with pytest.raises(EngineError, match="error -4.*" + option):
            e2.thermal_solve(np.zeros((int(model["npts_nonempty"]), int(model["nlevels"]))))
        with pytest.raises(EngineError, match="error -4"):
            e2.grid_update_thermal(ts, thick=cs["thick"])
        e2.close()
