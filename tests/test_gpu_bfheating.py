"""The bound-free heating coefficients on the device (artis_amd_bfheating_*, artis_amd_thermal_solve_bfheated, artis_amd_debug_gk61)
against the x86 build of the same rules (tests/bfheat_host) applied to the downloaded estimators, fit and cell state. The integrand takes
the stage's own exp and expm1 and every other operation is +, -, x, / in one order, so every coefficient, renormalisation factor, flag
and total must be the same bits on both machines. Models: synth "tiny" on 4 cells per axis (2 elements, 12 table points, the smallest
with two-target levels; every cell fitted), "small" on 8 per axis with a thick core, and "small" on a 1D grid."""
import ctypes as C

import numpy as np
import pytest

import bfheat_common as bc
import thermal_common as tc
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
NPK = 20000
CASES = [dict(id="tiny_3d", kind="tiny", gridtype=abi.GRID_CARTESIAN3D), dict(id="small_3d_thick_core", kind="small", gridtype=abi.GRID_CARTESIAN3D),
         dict(id="small_1d", kind="small", gridtype=abi.GRID_SPHERICAL1D)]


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


class Run:
    """one model, its packets and a host mirror of the cell state"""

    def __init__(self, kind="small", gridtype=abi.GRID_CARTESIAN3D):
        if kind == "tiny":
            model, cs0, _, aux = synth.build("tiny", ncoord=4, gridtype=gridtype, nts=10)
            self.model = synth.with_meannucmass(model)
        else:
            self.model, cs0, _, aux = tc.build_model(gridtype)
        self.pk0 = synth.make_packets(self.model, aux, NPK, kpkt_fraction=0.2, ts_width_frac=(1.0 + tc.WIDTH) ** 4 - 1.0)
        self.state = dict(cs0.d)
        self.ts = synth.make_timestep(aux["t"], width_frac=tc.WIDTH, vmax=self.model["vmax"], nts=10)
        self.ts_next = tc.next_timestep(self.model, self.ts)
        self.nm = synth.next_matter(self.model, abi.CellState(self.state), self.ts.c.mid, self.ts_next.c.mid, "classic")
        self.hm = bc.HostModel(self.model)
        self.vol = synth.assocvolume_tmin(self.model)

    def engine(self, engine_mod, preset="classic"):
        eng = engine_mod.Engine(self.model, preset=preset)
        eng.set_cellstate(abi.CellState(self.state), self.ts)
        eng._npk = NPK
        return eng

    def fit(self, eng):
        return eng.radfield_fit(self.ts.c.mid, self.ts.c.width, self.vol, lte_iteration=False)

    def step_and_fit(self, eng):
        eng.upload_packets(self.pk0)
        eng.step()
        return self.fit(eng)

    def estimators(self, eng):
        est = abi.Estimators(self.hm.n, self.hm.g)
        eng.download_estimators(est)
        return est

    def inputs(self, eng, fit, TR=None, W=None):
        """the x86 rules' inputs from the engine's estimators and fit"""
        raw = np.asarray(self.estimators(eng).bfheatingestimator).reshape(self.hm.n, self.hm.g).copy()
        return bc.call_inputs(self.model, self.state, self.ts, fit, raw, self.vol, TR, W)

    def heating(self):
        n = self.hm.n
        return dict(rho=self.nm["rho"], elem_massfracs=self.nm["elem_massfracs"], ntlepton_dep=np.full(n, 1e-9), dep_alpha=np.full(n, 1e-11),
                    dep_spfission=np.zeros(n))


def _same(d, h, label):
    for k in ("coeffs", "renorm", "flags"):
        assert d[k].shape == h[k].shape and d[k].tobytes() == h[k].tobytes(), (label, k, int((d[k] != h[k]).sum()))
    assert d["totals"] == h["totals"], (label, d["totals"], h["totals"])


@pytest.fixture(scope="module", params=CASES, ids=[c["id"] for c in CASES])
def updated(engine_mod, request):
    """one step, fit and update of a case on the device, and the x86 rules on the downloaded inputs"""
    case = request.param
    run = Run(case["kind"], case["gridtype"])
    eng = run.engine(engine_mod)
    fit = run.step_and_fit(eng)
    d = eng.bfheating_update()
    ins = run.inputs(eng, fit)
    yield dict(case=case, run=run, eng=eng, fit=fit, ins=ins, d=d, h=run.hm.update(ins), fitted=(fit["flags"] & abi.RADFIELD_FITTED) != 0)
    eng.close()


def test_device_matches_x86_bit_for_bit(updated):
    case, run, d, h, fitted = (updated[k] for k in ("case", "run", "d", "h", "fitted"))
    label = case["id"]
    nt = np.asarray(run.model.d["level_nphixstargets"])
    print(f"{label}: {int(fitted.sum())} fitted cells of {run.hm.n}, {int((nt > 0).sum())} levels with targets ({int((nt > 1).sum())} with two or more), "
          f"{d['nintegrals']} integrals, totals {d['totals']}, kernel ms {d['kernel_ms']}")
    assert d["nfitted"] == fitted.sum() > 0 and (nt > 1).any()
    if case["id"] == "small_3d_thick_core":  # thick and thin cells side by side: the boundary is in the comparison
        assert 0 < fitted.sum() < run.hm.n
    if case["kind"] == "tiny":
        assert fitted.all()
    _same(d, h, label)
    assert d["nlevels_with_targets"] == run.hm.nlisted and d["totals"]["nodes"] >= d["nintegrals"]
    # (a coefficient is 0 where the Monte Carlo estimator of its ground continuum is: no packet was absorbed there in the step)
    assert np.isfinite(d["coeffs"]).all() and (d["coeffs"] >= 0).all() and (d["coeffs"][fitted][:, nt > 0] > 0).any(axis=1).all()
    assert not d["coeffs"][~fitted].any() and not np.signbit(d["coeffs"]).any() and not d["coeffs"][:, nt == 0].any()
    # the ground integrals read the resident field, the levels the fit's: the fit has moved T_R or W in the fitted cells
    moved = (np.asarray(run.state["TR"], np.float32) != updated["fit"]["TR"]) | (np.asarray(run.state["W"], np.float32) != updated["fit"]["W"])
    assert moved[fitted].any()


def test_edge_cells_through_the_overrides(updated):
    """W = 0, T_R = MINTEMP and T_R = MAXTEMP (small expm1 arguments) in three fitted cells: bit-identical to x86 and finite"""
    run, eng, fit, fitted = (updated[k] for k in ("run", "eng", "fit", "fitted"))
    L = tc.lib()
    cells = np.nonzero(fitted)[0][[0, len(np.nonzero(fitted)[0]) // 2, -1]]
    TR, W = np.array(fit["TR"], np.float32), np.array(fit["W"], np.float32)
    W[cells[0]] = 0.0
    TR[cells[1]], TR[cells[2]] = L.tb_host_mintemp(), L.tb_host_maxtemp()
    d = eng.bfheating_update(TR=TR, W=W)
    h = run.hm.update(run.inputs(eng, fit, TR, W))
    _same(d, h, updated["case"]["id"])
    nt = np.asarray(run.model.d["level_nphixstargets"])
    assert np.isfinite(d["coeffs"]).all() and not d["coeffs"][cells[0]].any() and (d["coeffs"][cells[2]][nt > 0] > 0).any()
    assert not np.array_equal(d["coeffs"][cells[1]], updated["d"]["coeffs"][cells[1]])
    # the factors come from the resident field: the overrides do not reach them
    assert d["renorm"].tobytes() == updated["d"]["renorm"].tobytes()


def test_update_leaves_everything_else_alone(updated):
    """estimators, packets and counters byte-identical before and after an update; the resident cell state as far as the engine shows
    it: the rates of the resident state (artis_amd_thermal_rates without the ion balance reads T_e, n_e, populations, partition functions
    and T_J) and the factors, which read the resident T_R and W"""
    run, eng = updated["run"], updated["eng"]
    n, nl = run.hm.n, run.hm.nl
    heat = {k: v for k, v in run.heating().items() if k not in ("rho", "elem_massfracs")}

    def snapshot():
        pk = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
        eng.download_packets(pk)
        est = run.estimators(eng)
        r = eng.thermal_rates(np.ones((n, nl)), Te=None, rebalance=False, **heat)
        blobs = [pk.tobytes(), np.asarray(est.stats).tobytes()]
        blobs += [np.asarray(getattr(est, k)).tobytes() for k in ("J", "nuJ", "ffheatingestimator", "colheatingestimator", "gammaestimator", "bfheatingestimator")]
        blobs += [r[k].tobytes() for k in ("Te", "nne", "ion_groundlevelpops", "rates")]
        return blobs

    before = snapshot()
    a = eng.bfheating_update()
    after = snapshot()
    b = eng.bfheating_update()
    assert before == after
    for k in ("coeffs", "renorm", "flags"):
        assert a[k].tobytes() == b[k].tobytes() == updated["d"][k].tobytes(), k
    assert a["totals"] == b["totals"]


def test_debug_gk61_matches_the_golden_file(engine_mod):
    """the subdividing walk on the device, one lane per case of set (a): result, error estimate and evaluation count bit for bit"""
    gold = bc.golden()["analytic"]
    got = engine_mod.debug_gk61(bc.golden_analytic_cases())
    fh = float.fromhex
    for c, r in zip(gold, got):
        assert r["result"].hex() == fh(c["result"]).hex() and r["error"].hex() == fh(c["error"]).hex() and r["evals"] == c["evaluations"], (c, r)
        assert r["evals"] == bc.NODE * r["nodes"]
    depths = np.array([r["maxdepth"] for r in got])
    assert ((depths >= 3) & (depths < bc.MAX_DEPTH)).sum() >= 3 and (depths == bc.MAX_DEPTH).sum() >= 1


def _copy_estimators(src, dst):
    """src's estimator block over dst's, device to device (the sums of two runs' atomics differ in their last bits)"""
    import torch  # (the HIP runtime the process already has)

    (pa, na), (pb, nb) = src.estimators_devptr(), dst.estimators_devptr()
    assert na == nb
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    assert hip.hipMemcpy(pb, pa, 8 * na, 3) == 0  # hipMemcpyDeviceToDevice


def test_solve_bfheated_is_the_solve_on_the_downloaded_array(engine_mod):
    """thermal_solve_bfheated() and thermal_solve() handed the stage's own download: identical bytes in every array of the thermal
    download; grid_update_thermal() then succeeds, and a following step of two engines taken the two ways gives identical packets and
    counters"""
    run = Run()
    ea, eb = run.engine(engine_mod), run.engine(engine_mod)
    for eng in (ea, eb):
        eng.upload_packets(run.pk0)
        eng.step()
    _copy_estimators(ea, eb)
    fa, fb = run.fit(ea), run.fit(eb)
    assert all(fa[k].tobytes() == fb[k].tobytes() for k in ("TR", "W", "TJ", "flags"))
    bf = ea.bfheating_update()
    heat = run.heating()
    ta = ea.thermal_solve_bfheated(**heat)
    tb = eb.thermal_solve(bf["coeffs"], **heat)
    ta2 = ea.thermal_solve(bf["coeffs"], **heat)  # (and on the same engine)
    for k, v in ta.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == tb[k].tobytes() == ta2[k].tobytes(), k
    assert ta["ncells_flagged"] == tb["ncells_flagged"] and ta["total_evals"] == tb["total_evals"] and ta["nfitted"] == bf["nfitted"]
    assert (ta["rates"][:, 5] > 0).any()  # (heating_bf from the stage's block)
    ea.thermal_solve_bfheated(**heat)
    da = ea.grid_update_thermal(run.ts_next, thick=run.nm["thick"])
    db = eb.grid_update_thermal(run.ts_next, thick=run.nm["thick"])
    assert np.array_equal(da["Te"], ta["Te"]) and da["Te"].tobytes() == db["Te"].tobytes()
    outs = []
    for eng in (ea, eb):
        eng.zero_estimators()
        eng.step()
    for eng in (ea, eb):
        p = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
        eng.download_packets(p)
        outs.append((p, run.estimators(eng)))
        eng.close()
    (pa, sa), (pb, sb) = outs
    assert pa.tobytes() == pb.tobytes() and np.array_equal(sa.stats, sb.stats)


def test_refusals(engine_mod):
    from artis_amd.engine import EngineError

    run = Run("tiny")
    eng = run.engine(engine_mod)
    eng.upload_packets(run.pk0)
    eng.step()
    heat = run.heating()
    with pytest.raises(EngineError, match="error -3"):  # no fit since the last step
        eng.bfheating_update()
    with pytest.raises(EngineError, match="error -3"):  # nothing to download, nothing to solve with
        eng.bfheating_download()
    run.fit(eng)
    with pytest.raises(EngineError, match="error -3"):  # no update yet
        eng.thermal_solve_bfheated(**heat)
    with pytest.raises(EngineError, match="error -3"):  # T_R without W
        eng.bfheating_update(TR=np.full(run.hm.n, 5000.0))
    bf = eng.bfheating_update()
    with pytest.raises(EngineError, match="error -3"):  # an array handed to the call that reads the stage's block
        p, keep = abi.thermal_params(bf["coeffs"], heat["rho"], heat["elem_massfracs"], None, heat["ntlepton_dep"], heat["dep_alpha"], heat["dep_spfission"])
        eng._check(eng.L.artis_amd_thermal_solve_bfheated(eng.h, C.byref(p), None))
    with pytest.raises(EngineError, match="error -3"):  # artis_amd_thermal_solve itself still wants its array
        eng.thermal_solve(None, **heat)
    eng.thermal_solve_bfheated(**heat)
    eng.set_cellstate(abi.CellState(run.state), run.ts)
    with pytest.raises(EngineError, match="error -3.*resident cell state"):  # a cell state set since the update
        eng.thermal_solve_bfheated(**heat)
    eng.bfheating_update()
    eng.thermal_solve_bfheated(**heat)
    run.fit(eng)
    with pytest.raises(EngineError, match="error -3.*last artis_amd_radfield_fit"):  # a fit newer than the update
        eng.thermal_solve_bfheated(**heat)
    eng.close()
    model, cs, ts, aux = synth.build("small", ncoord=6, options="kilonova_lte")
    e2 = engine_mod.Engine(synth.with_meannucmass(model), preset="kilonova_lte")
    e2.set_cellstate(cs, ts)
    with pytest.raises(EngineError, match="error -4.*DIRECT_COL_HEAT"):
        e2.bfheating_update()
    with pytest.raises(EngineError, match="error -4"):
        e2.bfheating_download()
    with pytest.raises(EngineError, match="error -4"):
        e2.thermal_solve_bfheated()
    e2.close()

