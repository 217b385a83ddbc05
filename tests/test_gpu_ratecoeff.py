"""The rate-coefficient tables on the device (artis_amd_ratecoeff_*) against the x86 build of the same rules (tests/ratecoeff_host) with
the stage's own exp and expm1: every other operation is +, -, x, / in one order, so every entry, flag and total must be the same bits on
both machines. Then the call's batching, what it leaves alone, install against hand-in, and its refusals. Model: synth "small" on 6 cells
per axis (159 continua, levels with two targets) with the options of classic, kilonova_lte (interpolated cross-sections, 200
temperatures) and nltenebular (no USE_LUT_PHOTOION: two tables)."""
import ctypes as C

import numpy as np
import pytest

import ratecoeff_common as rc
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
NPK = 2000
WIDTH = 0.05
PRESETS = ("classic", "kilonova_lte", "nltenebular")


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


def _engine_model(preset):
    m = rc.model(preset)
    return m if preset.startswith("kilonova") else synth.with_meannucmass(m)


@pytest.fixture(scope="module", params=PRESETS)
def computed(engine_mod, request):
    """an engine that has only been created, its tables, and the x86 rules on the same model (made once, never changed)"""
    preset = request.param
    eng = engine_mod.Engine(_engine_model(preset), preset=preset)
    d = eng.ratecoeff_tables()
    hm = rc.HostModel(rc.model(preset), preset)
    yield dict(preset=preset, eng=eng, d=d, hm=hm, h=hm.tables(rc.TBMATH, shared=True))
    eng.close()


def test_device_matches_x86_bit_for_bit(computed):
    d, h, hm = computed["d"], computed["h"], computed["hm"]
    print(f"{computed['preset']}: {d['nbfcontinua']} continua x {d['tablesize']} temperatures, {d['ntables']} tables, {d['integrals']} integrals, "
          f"{d['nodes']} nodes, kernel {d['kernel_ms']:.3f} ms")
    assert (d["nbfcontinua"], d["tablesize"], d["ntables"], d["ncovered"]) == (hm.nbf, hm.tablesize, hm.ntables, hm.ncovered)
    assert d["ntables"] == (2 if computed["preset"] == "nltenebular" else 3)
    rc.same_tables(d, h, computed["preset"])
    assert {k: d[k] for k in rc.TOTALS} == h["totals"]
    assert d["integrals"] == d["nodes"] == hm.ntables * hm.ncovered * hm.tablesize and d["at_depth_cap"] == 0
    assert d["flagged"] == 0 and d["first_flagged"] == -1 and not d["flags"].any()
    for k in rc.TABLES:
        if d[k] is not None:
            assert np.isfinite(d[k]).all() and (d[k] >= 0).all() and d[k].any(axis=1).all()


def test_batching_leaves_every_byte(computed):
    """1000 entries per launch is no multiple of 64, 100 or 200: batch and wave boundaries fall inside a continuum; 37 entries per launch
    are launches of less than a wave"""
    eng, d = computed["eng"], computed["d"]
    for per_launch in (1000, 37):
        b = eng.ratecoeff_tables(items_per_launch=per_launch)
        rc.same_tables(b, d, (computed["preset"], per_launch))
        assert {k: b[k] for k in rc.TOTALS} == {k: d[k] for k in rc.TOTALS}


def test_cut_down_model(engine_mod, monkeypatch):
    """a model cut down to one ionising ion of three levels: three continua, 300 entries -- a table's rows come in whole temperature
    grids, so fewer than 64 entries do not exist; a launch of fewer does (37 per launch above, and 50 here: half a row)"""
    monkeypatch.setitem(synth.PRESETS, "one_ion", ([(14, 1, 2)], 3, 1.0, 12))
    m = synth.with_meannucmass(synth.build("one_ion", ncoord=4)[0])
    eng = engine_mod.Engine(m)
    d, half = eng.ratecoeff_tables(), eng.ratecoeff_tables(items_per_launch=50)
    eng.close()
    hm = rc.HostModel(m, "classic")
    assert hm.nbf == hm.ncovered == d["ncovered"] == 3 and d["integrals"] == d["nodes"] == 900
    h = hm.tables(rc.TBMATH)
    rc.same_tables(d, h, "one ion")
    rc.same_tables(half, h, "one ion, 50 per launch")
    assert all((d[k] > 0).all() for k in rc.TABLES)


class Run:
    """the classic small model with packets and a timestep"""

    def __init__(self, tables=None):
        model, cs, ts, aux = synth.build("small", ncoord=6, nts=10)
        self.base = synth.with_meannucmass(model)
        self.cs, self.aux = cs, aux
        self.ts = synth.make_timestep(aux["t"], width_frac=WIDTH, vmax=model["vmax"], nts=10)
        self.pk0 = synth.make_packets(model, aux, NPK, kpkt_fraction=0.2, ts_width_frac=(1.0 + WIDTH) ** 4 - 1.0)
        self.n, self.g = int(model["npts_nonempty"]), int(model["nbfcontinua_ground"])
        self.vol = synth.assocvolume_tmin(model)

    def model_with(self, tables) -> abi.Model:
        """the model with the three tables replaced (None: zeros, what a host that will install hands in)"""
        size = len(self.base["spontrecombcoeffs"])
        return rc.changed(self.base, **{k: (np.zeros(size) if tables is None else tables[k].ravel()) for k in rc.TABLES})

    def step(self, eng):
        """set_cellstate and one update_packets of the run's packets: (packets, estimators)"""
        eng.set_cellstate(self.cs, self.ts)
        pk = self.pk0.copy()
        est = abi.Estimators(self.n, self.g)
        eng.update_packets(pk, est)
        return pk, est


def _same_step(a, b, label):
    (pa, sa), (pb, sb) = a, b
    for f in abi.PACKET_DTYPE.names:  # every field, the generator states among them (the struct's padding is not data: the host-buffer
        assert pa[f].tobytes() == pb[f].tobytes(), (label, f)  # form of the call does not carry it)
    assert np.array_equal(sa.stats, sb.stats), label
    # the estimators are sums of device-wide f64 atomics, whose order differs from run to run: the bar the stage tests use between two runs
    for k in ("J", "nuJ", "ffheatingestimator", "colheatingestimator", "gammaestimator", "bfheatingestimator"):
        x, y = np.asarray(getattr(sa, k)), np.asarray(getattr(sb, k))
        assert np.array_equal(x == 0, y == 0), (label, k)
        assert np.all(np.abs(x - y) <= 1e-12 * np.abs(x)), (label, k)


def test_compute_without_install_leaves_the_engine_alone(engine_mod):
    run = Run()
    ea, eb = engine_mod.Engine(run.base), engine_mod.Engine(run.base)
    eb.ratecoeff_tables()  # before the cell state ...
    eb.set_cellstate(run.cs, run.ts)
    eb.ratecoeff_tables()  # ... and after it
    outs = [run.step(ea), run.step(eb)]
    ea.close()
    eb.close()
    _same_step(outs[0], outs[1], "no install")
    assert outs[0][0]["pos"].tobytes() != run.pk0["pos"].tobytes()


def test_install_equals_hand_in(engine_mod):
    """engine B is created with zeroed tables and installs; engine A is created with the downloaded tables handed in. set_cellstate, one
    update_packets and one grid_update (which reads ion_alpha_sp, made from spontrecombcoeffs) then agree"""
    run = Run()
    eb = engine_mod.Engine(run.model_with(None))
    installed = eb.ratecoeff_tables(install=True)
    assert all((installed[k] > 0).all() for k in rc.TABLES)
    ea = engine_mod.Engine(run.model_with(installed))
    outs, balances = [], []
    ts_next = synth.make_timestep(run.ts.c.start + run.ts.c.width, width_frac=WIDTH, vmax=run.base["vmax"], nts=run.ts.c.nts + 1)
    nm = synth.next_matter(run.base, run.cs, run.ts.c.mid, ts_next.c.mid, "classic")
    for eng in (ea, eb):
        outs.append(run.step(eng))
    # (the balance reads the estimators: give both engines the same sums, as the other stage tests do between two runs)
    _copy_estimators(ea, eb)
    for eng in (ea, eb):
        eng.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol, lte_iteration=False)
        balances.append(eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], nm["thick"]))
        eng.close()
    _same_step(outs[0], outs[1], "install")
    for k, v in balances[0].items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == balances[1][k].tobytes(), k
    assert balances[0]["ncells_flagged"] == balances[1]["ncells_flagged"] and balances[0]["total_evals"] == balances[1]["total_evals"]
    assert (balances[0]["phi"] > 0).any()
    # and the zeroed tables do differ: an engine left with them propagates otherwise
    ez = engine_mod.Engine(run.model_with(None))
    pz, _ = run.step(ez)
    ez.close()
    assert pz["rngstate"].tobytes() != outs[0][0]["rngstate"].tobytes()


def _copy_estimators(src, dst):
    """src's estimator block over dst's, device to device (the sums of two runs' atomics differ in their last bits)"""
    import torch  # (the HIP runtime the process already has)

    (pa, na), (pb, nb) = src.estimators_devptr(), dst.estimators_devptr()
    assert na == nb
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    assert hip.hipMemcpy(pb, pa, 8 * na, 3) == 0  # hipMemcpyDeviceToDevice


def test_refusals(engine_mod):
    from artis_amd.engine import EngineError

    run = Run()
    eng = engine_mod.Engine(run.base)
    with pytest.raises(EngineError, match="error -3.*nothing computed"):
        eng.ratecoeff_download()
    req = abi.RatecoeffRequest(struct_size=C.sizeof(abi.RatecoeffRequest) - 8)
    with pytest.raises(EngineError, match="error -3.*struct_size"):
        eng._check(eng.L.artis_amd_ratecoeff_compute(eng.h, C.byref(req)))
    stats = abi.RatecoeffStats(struct_size=1)
    with pytest.raises(EngineError, match="error -3.*struct_size"):
        eng._check(eng.L.artis_amd_ratecoeff_download(eng.h, None, None, None, None, C.byref(stats)))
    with pytest.raises(EngineError, match="error -3.*items_per_launch"):
        eng.ratecoeff_tables(items_per_launch=-1)
    eng.ratecoeff_tables(install=True)  # set-up phase: allowed, and again
    eng.ratecoeff_tables(install=True)
    eng.set_cellstate(run.cs, run.ts)
    with pytest.raises(EngineError, match="error -3.*cell state"):
        eng.ratecoeff_tables(install=True)
    eng.ratecoeff_tables()  # computing is still allowed
    eng.close()
    # install after a grid_update: the cell state has changed AND ion_alpha_sp exists; the text names the first
    eng = engine_mod.Engine(run.base)
    run.step(eng)
    eng.radfield_fit(run.ts.c.mid, run.ts.c.width, run.vol, lte_iteration=False)
    ts_next = synth.make_timestep(run.ts.c.start + run.ts.c.width, width_frac=WIDTH, vmax=run.base["vmax"], nts=run.ts.c.nts + 1)
    nm = synth.next_matter(run.base, run.cs, run.ts.c.mid, ts_next.c.mid, "classic")
    eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], nm["thick"])
    with pytest.raises(EngineError, match="error -3.*install after"):
        eng.ratecoeff_tables(install=True)
    eng.close()
    # a corrphotoion pointer in a build without USE_LUT_PHOTOION
    e2 = engine_mod.Engine(_engine_model("nltenebular"), preset="nltenebular")
    d = e2.ratecoeff_tables()
    assert d["corrphotoioncoeffs"] is None
    buf = np.zeros(d["nbfcontinua"] * d["tablesize"])
    with pytest.raises(EngineError, match="error -3.*USE_LUT_PHOTOION"):
        e2._check(e2.L.artis_amd_ratecoeff_download(e2.h, None, buf.ctypes.data_as(C.c_void_p), None, None, None))
    e2.close()
