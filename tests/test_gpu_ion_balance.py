"""The ion balance and hand-over of the grid update on the device (artis_amd_grid_update*), against the x86 build of the same rules
(tests/ionbal_host) applied to the downloaded estimators and cell state, on the synthetic models. A float that the device's exp / pow
moves by one ulp is allowed and counted; a cell whose partition functions differ in a last bit may take another path through the
root search, so its n_e is held to the search's tolerance and its populations to the rules at the device's own root. The state
the call leaves must propagate packets exactly as the same arrays handed over through artis_amd_set_cellstate."""
import numpy as np
import pytest

import ionbal_common as ib
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
WIDTH = 0.05
NPK = 20000


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


class Run:
    """one engine over several timesteps, with a host mirror of its cell state"""

    def __init__(self, engine_mod, preset, gridtype=abi.GRID_CARTESIAN3D, thick_below_v=0.0, npk=NPK, nsteps_max=4):
        model, cs0, ts0, aux = synth.build("small", ncoord=8, gridtype=gridtype, options=preset, nts=10, thick_below_v=thick_below_v)
        if not preset.startswith("kilonova"):
            model = synth.with_meannucmass(model)
        self.model, self.preset, self.aux = model, preset, aux
        self.pk0 = synth.make_packets(model, aux, npk, kpkt_fraction=0.2, ts_width_frac=(1.0 + WIDTH) ** nsteps_max - 1.0)
        self.state = dict(cs0.d)
        self.t = aux["t"]
        self.ts = synth.make_timestep(self.t, width_frac=WIDTH, vmax=model["vmax"], nts=10)
        self.host = ib.HostModel(model, preset)
        self.vol = synth.assocvolume_tmin(model)
        if preset.startswith("kilonova") and self.state.get("elem_meanweight") is None:
            self.state["elem_meanweight"] = synth.next_matter(model, cs0, self.t, self.t, preset)["elem_meanweight"]

    def engine(self, engine_mod):
        eng = engine_mod.Engine(self.model, preset=self.preset)
        eng.set_cellstate(abi.CellState(self.state), self.ts)
        return eng

    def next_ts(self):
        t1 = self.ts.c.start + self.ts.c.width
        return synth.make_timestep(t1, width_frac=WIDTH, vmax=self.model["vmax"], nts=self.ts.c.nts + 1)

    def host_expect(self, eng, d_fit, use_fit, lte, nm, host_T=None, Te_override=None):
        """the x86 rules on the downloaded estimators and the mirrored current state"""
        n, g = int(self.model["npts_nonempty"]), int(self.model["nbfcontinua_ground"])
        if use_fit:
            est = abi.Estimators(n, g)
            eng.download_estimators(est)
            gamma = ib.gamma_normed(np.asarray(est.gammaestimator).reshape(n, g), self.vol, self.ts.c.mid, float(self.model["tmin"]),
                                    self.ts.c.width)
            TJ, Te = d_fit["TJ"], d_fit["Te"].copy()
            if Te_override is not None:
                fitted = (d_fit["flags"] & abi.RADFIELD_FITTED) != 0
                Te[fitted] = Te_override[fitted]
        else:
            gamma = np.zeros((n, g))
            TJ, Te = host_T["TJ"], host_T["Te"]
        thick_cur = np.asarray(self.state["thick"])
        forced = (np.full(n, bool(lte)) | (thick_cur == ib.CELL_THICK)).astype(np.int32)
        clump = np.asarray(self.state["clumpfactor"], np.float32)
        h = self.host.balance(TJ, Te, forced, self.state["ion_groundlevelpops"], nm["elem_massfracs"], nm["elem_meanweight"], nm["rho"],
                              clump, gamma, nthreads=16)
        h["gamma"], h["forced"] = gamma, forced
        return h

    def compare(self, d, h, label):
        n = int(self.model["npts_nonempty"])
        assert np.array_equal(d["gamma_normed"], h["gamma"]), label
        assert np.array_equal(d["nnetot"], h["nnetot"]), label
        assert np.array_equal((d["flags"] & abi.IONBAL_FORCED_SAHA) != 0, h["forced"] != 0), label
        uU = _ulps(d["ion_partfuncts"], h["U"])
        assert uU.max() <= 1, (label, int(uU.max()))
        # phi: a few ulps where the device's exp / pow (phi_saha, the ion_alpha_sp weights) differ from glibc's in a last bit
        with np.errstate(invalid="ignore"):  # (phi is inf above an ion without photoionisation)
            rphi = np.abs(d["phi"] / np.where(h["phi"] == 0, 1, h["phi"]) - 1)
        rphi = np.where(d["phi"] == h["phi"], 0, rphi)[(uU == 0).all(axis=1)]
        assert np.nanmax(rphi, initial=0) <= 1e-13, (label, float(np.nanmax(rphi, initial=0)))
        same = (uU == 0).all(axis=1) & (d["phi"] == h["phi"]).all(axis=1)
        # cells whose partition functions and phi are bit-identical: everything identical
        for k_d, k_h in (("ion_groundlevelpops", "ground"), ("uppermost_ion", "uppermost"), ("nne", "nne"), ("nne_root", "nne_root"),
                         ("evals", "evals"), ("flags", "flags")):
            assert np.array_equal(d[k_d][same], h[k_h][same]), (label, k_d)
        # the others: the same uppermost ions, n_e to the root search's tolerance
        diff = ~same
        assert np.array_equal(d["uppermost_ion"], h["uppermost"]), label
        if diff.any():
            rel = np.abs(d["nne"][diff].astype(np.float64) / h["nne"][diff] - 1)
            assert rel.max() <= 2e-3, (label, float(rel.max()))
        print(f"{label}: {int(diff.sum())} of {n} cells with U or phi apart in a last bit ({int((uU == 1).sum())} U, "
              f"{int((d['phi'] != h['phi']).sum())} phi entries), "
              f"flags {d['ncells_flagged']}, {d['total_evals']} residual evaluations")

    def handover_state(self, d, nm):
        """the arrays the call wrote into the engine's cell state, as a host would hand them over through set_cellstate"""
        s = dict(self.state)
        for k in ("Te", "TJ", "TR", "W", "nne", "nnetot", "rho"):
            s[k] = d[k]
        s["ion_partfuncts"] = d["ion_partfuncts"].ravel()
        s["ion_groundlevelpops"] = d["ion_groundlevelpops"].ravel()
        s["elem_massfracs"] = nm["elem_massfracs"]
        s["thick"] = nm["thick"]
        if nm["elem_meanweight"] is not None:
            s["elem_meanweight"] = nm["elem_meanweight"]
        g = int(self.model["nbfcontinua_ground"])
        renorm = np.asarray(s["corrphotoionrenorm"], np.float64).reshape(-1, max(g, 1)).copy()
        renorm[(d["flags"] & abi.IONBAL_FORCED_SAHA) != 0] = 1.0
        s["corrphotoionrenorm"] = renorm.ravel()
        return s


def _step_and_compare(ea, eb, model, label):
    """one step of both engines from the same packets and zeroed estimators: packets, counters and estimators identical"""
    n, g = int(model["npts_nonempty"]), int(model["nbfcontinua_ground"])
    outs = []
    for eng in (ea, eb):
        eng.zero_estimators()
        eng.step()
    for eng in (ea, eb):
        p = np.zeros(ea._npk, dtype=abi.PACKET_DTYPE)
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


def _grid_update(run, eng, lte, use_fit=True, Te_override=None):
    """fit (use_fit) and grid_update of one engine; returns (download, host rules, next matter, next timestep)"""
    ts_next = run.next_ts()
    nm = synth.next_matter(run.model, abi.CellState(run.state), run.ts.c.mid, ts_next.c.mid, run.preset)
    host_T = None
    if use_fit:
        d_fit = eng.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol, lte_iteration=lte)
        h = run.host_expect(eng, d_fit, True, lte, nm, Te_override=Te_override)
        d = eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], nm["thick"], use_fit=True, elem_meanweight=nm["elem_meanweight"],
                            Te=Te_override)
    else:
        host_T = dict(TJ=np.asarray(run.state["TJ"], np.float32) * np.float32(1.03), Te=np.asarray(run.state["TJ"], np.float32) * np.float32(1.03))
        h = run.host_expect(eng, None, False, True, nm, host_T=host_T)
        d = eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], nm["thick"], use_fit=False, elem_meanweight=nm["elem_meanweight"],
                            TJ=host_T["TJ"], TR=host_T["TJ"], W=np.ones_like(host_T["TJ"]), Te=host_T["Te"])
    return d, h, nm, ts_next


CASES = [
    dict(id="classic_nebular_thick", preset="classic", thick_below_v=1e9, lte=False),
    dict(id="classic_lte", preset="classic", lte=True),
    dict(id="kilonova_lte", preset="kilonova_lte", lte=False),
    dict(id="classic_1d", preset="classic", gridtype=abi.GRID_SPHERICAL1D, lte=False),
    dict(id="classic_use_fit0", preset="classic", use_fit=False, lte=True),
]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_grid_update_matches_host_rules_and_hands_over(engine_mod, case):
    run = Run(engine_mod, case["preset"], gridtype=case.get("gridtype", abi.GRID_CARTESIAN3D), thick_below_v=case.get("thick_below_v", 0.0))
    ea, eb = run.engine(engine_mod), run.engine(engine_mod)
    ea._npk = NPK
    ea.upload_packets(run.pk0)
    ea.step()
    d, h, nm, ts_next = _grid_update(run, ea, case["lte"], use_fit=case.get("use_fit", True))
    run.compare(d, h, case["id"])
    if case["id"] == "classic_nebular_thick":
        assert d["ncells_flagged"]["forced_saha"] > 0 and d["ncells_flagged"]["forced_saha"] < run.model["npts_nonempty"]
    # two calls on the same state are identical (a fresh fit on the same estimators for the second)
    pk = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
    ea.download_packets(pk)
    # the hand-over: engine B gets A's result through set_cellstate; the next step from the same packets is identical
    eb.set_cellstate(abi.CellState(run.handover_state(d, nm)), ts_next)
    eb.upload_packets(pk)
    _step_and_compare(ea, eb, run.model, case["id"])
    ea.close()
    eb.close()


def test_two_calls_identical(engine_mod):
    run = Run(engine_mod, "classic", thick_below_v=1e9)
    eng = run.engine(engine_mod)
    eng.upload_packets(run.pk0)
    eng.step()
    eng.snapshot()
    outs = []
    for _ in range(2):
        ts_next = run.next_ts()
        nm = synth.next_matter(run.model, abi.CellState(run.state), run.ts.c.mid, ts_next.c.mid)
        eng.set_cellstate(abi.CellState(run.state), run.ts)  # the same state before each call
        eng.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol)
        outs.append(eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], nm["thick"]))
    for k in ("Te", "TJ", "nne", "nnetot", "ion_partfuncts", "ion_groundlevelpops", "uppermost_ion", "gamma_normed", "flags", "evals"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    eng.close()


def test_handover_with_tiled_cache(engine_mod, monkeypatch):
    run = Run(engine_mod, "classic", thick_below_v=1e9)
    probe = run.engine(engine_mod)
    _, _, bpc = probe.cache_tiles()
    probe.close()
    n = int(run.model["npts_nonempty"])
    monkeypatch.setenv("ARTIS_AMD_MA_HOTFRAC", "1")
    monkeypatch.setenv("ARTIS_AMD_MA_POOLFRAC", "1")
    monkeypatch.setenv("ARTIS_AMD_CACHE_BUDGET_MB", f"{bpc * n / 3 / 2**20:.3f}")
    ea, eb = run.engine(engine_mod), run.engine(engine_mod)
    assert ea.cache_tiles()[0] > 1 and eb.cache_tiles()[0] > 1
    ea._npk = NPK
    ea.upload_packets(run.pk0)
    ea.step()
    d, h, nm, ts_next = _grid_update(run, ea, False)
    run.compare(d, h, "tiled")
    pk = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
    ea.download_packets(pk)
    eb.set_cellstate(abi.CellState(run.handover_state(d, nm)), ts_next)
    eb.upload_packets(pk)
    _step_and_compare(ea, eb, run.model, "tiled")
    ea.close()
    eb.close()


def test_three_timesteps_on_the_device(engine_mod):
    """LTE, then two nebular timesteps with the host's T_e left as it is: step -> fit -> grid_update entirely on the device; at every
    timestep the state agrees with the x86 rules on that timestep's inputs, and a twin handed the same state propagates identically"""
    run = Run(engine_mod, "classic", thick_below_v=8e8)
    ea = run.engine(engine_mod)
    ea._npk = NPK
    ea.upload_packets(run.pk0)
    for k, lte in enumerate((True, False, False)):
        pk = np.zeros(NPK, dtype=abi.PACKET_DTYPE)
        ea.download_packets(pk)
        eb = run.engine(engine_mod)
        eb.upload_packets(pk)
        _step_and_compare(ea, eb, run.model, f"timestep {k}: twin")
        eb.close()
        d, h, nm, ts_next = _grid_update(run, ea, lte)
        run.compare(d, h, f"timestep {k}")
        run.state = run.handover_state(d, nm)
        run.ts = ts_next
    ea.close()


def test_refusals(engine_mod):
    from artis_amd.engine import EngineError

    run = Run(engine_mod, "classic")
    eng = run.engine(engine_mod)
    eng.upload_packets(run.pk0)
    eng.step()
    ts_next = run.next_ts()
    nm = synth.next_matter(run.model, abi.CellState(run.state), run.ts.c.mid, ts_next.c.mid)
    with pytest.raises(EngineError, match="error -3"):  # no fit since the last step
        eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], nm["thick"])
    with pytest.raises(EngineError, match="error -3"):  # use_fit = 0 without temperatures
        eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], nm["thick"], use_fit=False)
    eng.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol)
    with pytest.raises(EngineError, match="error -3"):  # no thick
        eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], None)
    eng.close()
    # a model without elem_meannucmass in a build that reads it
    model, cs, ts, aux = synth.build("small", ncoord=6)
    e2 = engine_mod.Engine(model)
    e2.set_cellstate(cs, ts)
    e2.upload_packets(synth.make_packets(model, aux, 2000))
    e2.step()
    e2.radfield_fit(ts.c.mid, ts.c.width, synth.assocvolume_tmin(model))
    with pytest.raises(EngineError, match="elem_meannucmass"):
        e2.grid_update(ts, cs["rho"], cs["elem_massfracs"], cs["thick"])
    e2.close()
    # the nebular family
    model, cs, ts, aux = synth.build("small", ncoord=6, options="nltenebular")
    e3 = engine_mod.Engine(synth.with_meannucmass(model), preset="nltenebular")
    e3.set_cellstate(cs, ts)
    with pytest.raises(EngineError, match="error -4"):
        e3.grid_update(ts, cs["rho"], cs["elem_massfracs"], cs["thick"])
    e3.close()
