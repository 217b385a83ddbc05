"""GPU tests of the absent-ion skip of the cell-cache population (DESIGN.md sections 2 and 3): the static macro-atom records of an ion whose
population in a cell is at most ARTIS_AMD_MA_ABSENT_EPS times its element's are left out -- they hold a marker -- and the slow-path kernel fills
such a record when a packet first reaches it, with the bits the population would have written. Which records are populated when is placement:
every field of every packet, the generator states and the event counters must be those of a run that populates everything (eps negative), the
estimators theirs to summation order (the tolerance of the other placement tests, 1e-11).

Shapes: the `small` atomic data on 8^3 and on 16 shells with a few thousand packets; mostly k-packets where the thermal lists have to reach the
4096 entries of the bulk form of k_thermal; a few hundred packets where k_late or k_tail are to end the population; a cache of two tiles; and
the bench's atomic data (`w7`) on 6^3 for the default's own skip."""
import numpy as np
import pytest

import parity
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu

VARIABLES = ("ARTIS_AMD_MA_ABSENT_EPS", "ARTIS_AMD_LATE", "ARTIS_AMD_LATE_ALWAYS", "ARTIS_AMD_LATE_STRICT", "ARTIS_AMD_TAIL_ALWAYS")
ALL_POPULATED = {"ARTIS_AMD_MA_ABSENT_EPS": "-1"}
NONE_POPULATED = {"ARTIS_AMD_MA_ABSENT_EPS": "1"}
DEFAULT = {}


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from artis_amd import engine

    engine.load_library()
    return engine


def run(engine_mod, monkeypatch, model, cs, ts, pk0, env, config=None):
    """one step of the packets on a new engine created under `env`"""
    for v in VARIABLES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_mod.Engine(model, config=config)
    tiles = eng.cache_tiles()
    eng.set_cellstate(cs, ts)
    p, e = pk0.copy(), abi.estimators_for(model, "classic")
    eng.update_packets(p, e)
    skipped, filled = eng.last_absent_records()
    out = dict(p=p, e=e, skipped=skipped, filled=filled, variants=eng.last_thermal_variants(), tiles=tiles, ms=eng.last_kernel_ms_by_kind())
    eng.close()
    return out


def same(got, want, what):
    parity.compare_packets(got["p"], want["p"], 0.0, what)
    assert np.array_equal(got["p"]["rngstate"], want["p"]["rngstate"]), what
    parity.compare_stats(got["e"], want["e"], what)
    parity.compare_estimators(got["e"], want["e"], 1e-11, what)


@pytest.mark.parametrize("gridtype,ncoord", [(abi.GRID_CARTESIAN3D, 8), (abi.GRID_SPHERICAL1D, 16)])
def test_default_eps_gives_the_packets_of_a_full_population(engine_mod, monkeypatch, gridtype, ncoord):
    model, cs, ts, aux = synth.build("small", ncoord=ncoord, gridtype=gridtype)
    pk0 = synth.make_packets(model, aux, 5000, kpkt_fraction=0.2)
    full = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALL_POPULATED)
    dflt = run(engine_mod, monkeypatch, model, cs, ts, pk0, DEFAULT)
    assert full["skipped"] == 0 and full["filled"] == 0
    print(f"small default eps: skipped {dflt['skipped']} filled {dflt['filled']}")  # (that the default leaves records out is asserted with the bench's data below)
    same(dflt, full, "default eps vs everything populated")


@pytest.mark.parametrize("gridtype,ncoord", [(abi.GRID_CARTESIAN3D, 8), (abi.GRID_SPHERICAL1D, 16)])
def test_every_record_filled_on_demand_gives_the_same_packets(engine_mod, monkeypatch, gridtype, ncoord):
    """eps = 1: no record is populated, every record a packet reaches is filled by the slow path; enough k-packets that the thermal lists are
    long enough for the bulk form of k_thermal (4096 entries: the LDS-table form), which is where the marker is then met"""
    model, cs, ts, aux = synth.build("small", ncoord=ncoord, gridtype=gridtype)
    pk0 = synth.make_packets(model, aux, 20000, kpkt_fraction=0.8)
    full = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALL_POPULATED)
    none = run(engine_mod, monkeypatch, model, cs, ts, pk0, NONE_POPULATED)
    bulk = engine_mod.Engine.THERMAL_LDS_TABLES | engine_mod.Engine.THERMAL_LDS_LEVELPACK
    assert none["variants"] & bulk, none["variants"]
    print(f"skipped {none['skipped']} filled {none['filled']}")
    assert none["filled"] > 0 and none["filled"] <= none["skipped"], (none["filled"], none["skipped"])
    same(none, full, "eps = 1 vs everything populated")


@pytest.mark.parametrize("end,env", [("k_late", {"ARTIS_AMD_LATE": "100000000", "ARTIS_AMD_LATE_ALWAYS": "1", "ARTIS_AMD_LATE_STRICT": "1"}),
                                     ("k_tail", {"ARTIS_AMD_LATE": "0", "ARTIS_AMD_TAIL_ALWAYS": "1"})])
def test_marker_met_in_the_kernels_that_end_a_population(engine_mod, monkeypatch, end, env):
    """so few packets that k_late / k_tail carry the population: a packet that meets the marker there leaves for the slow-path list"""
    model, cs, ts, aux = synth.build("small", ncoord=8)
    pk0 = synth.make_packets(model, aux, 600, kpkt_fraction=0.5)
    full = run(engine_mod, monkeypatch, model, cs, ts, pk0, {**env, **ALL_POPULATED})
    none = run(engine_mod, monkeypatch, model, cs, ts, pk0, {**env, **NONE_POPULATED})
    bit = engine_mod.Engine.THERMAL_LATE if end == "k_late" else engine_mod.Engine.THERMAL_TAIL
    assert full["variants"] & bit and none["variants"] & bit, (full["variants"], none["variants"])
    assert 0 < none["filled"] <= none["skipped"], (none["filled"], none["skipped"])
    same(none, full, f"eps = 1 vs everything populated, {end}")


def test_markers_are_rewritten_at_every_fill_of_a_tiled_cache(engine_mod, monkeypatch):
    model, cs, ts, aux = synth.build("small", ncoord=6)
    pk0 = synth.make_packets(model, aux, 6000, kpkt_fraction=0.5)
    base = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALL_POPULATED)
    assert base["tiles"][0] == 1
    two = dict(cache_budget_bytes=int(base["tiles"][2]) * (model["npts_nonempty"] // 2 + 1) + 4096, ma_hot_fraction=1.0, ma_pool_fraction=1.0)
    full = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALL_POPULATED, config=two)
    none = run(engine_mod, monkeypatch, model, cs, ts, pk0, NONE_POPULATED, config=two)
    assert full["tiles"][0] == 2 and none["tiles"][0] == 2
    assert none["filled"] > 0 and none["skipped"] > 0
    same(none, full, "eps = 1 vs everything populated, two tiles")
    same(none, base, "eps = 1 on two tiles vs one tile, everything populated")


def test_debug_view_fills_an_absent_record_before_reading_it(engine_mod, monkeypatch):
    """a cell in which no packet ran: the records artis_amd_debug_cellcache() returns are the population's, bit for bit"""
    model, cs, ts, aux = synth.build("small", ncoord=8)
    views = []
    for env in (ALL_POPULATED, NONE_POPULATED):
        for v in VARIABLES:
            monkeypatch.delenv(v, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = engine_mod.Engine(model)
        eng.set_cellstate(cs, ts)
        views.append((eng.debug_cellcache(model["npts_nonempty"] // 2), eng.last_absent_records()))
        eng.close()
    (full, (fs, _)), (none, (ns, _)) = views
    assert fs == 0 and ns > 0
    assert np.any(full["maprocessrates"] != 0.)
    for key in ("maprocessrates", "matrans", "levelpops", "cooling_contrib", "ion_cooling_contribs"):
        assert np.array_equal(full[key], none[key]), key


def test_default_eps_skips_records_of_the_bench_model(engine_mod, monkeypatch):
    """the bench's atomic data on 6^3: the default eps leaves records out (so the comparison is not one of two identical populations) and the
    packets are those of a full population"""
    model, cs, ts, aux = synth.build("w7", ncoord=6)
    pk0 = synth.make_packets(model, aux, 4000, kpkt_fraction=0.5)
    full = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALL_POPULATED)
    dflt = run(engine_mod, monkeypatch, model, cs, ts, pk0, DEFAULT)
    print(f"w7 6^3 default eps: skipped {dflt['skipped']} filled {dflt['filled']}")
    assert full["skipped"] == 0 and dflt["skipped"] > 0
    same(dflt, full, "default eps vs everything populated, w7")
