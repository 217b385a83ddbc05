"""GPU tests of the ways the kernels ADD UP the per-cell estimators, each against the CPU oracle with the per-entry bar of
parity.compare_estimators, and each form against the others on the device (run with `pytest -m gpu`).

Which form a kernel takes follows from the number of non-empty cells (rpkt_kernels.h: RPKT_CELLEST_CAP 512 with the
continuum table in LDS, RPKT_CELLEST_CAP_NOCONT 3072 without it, GAMMA_CELLEST_CAP 2048, THERMAL_CELLEST_CAP 4096) and from
the ARTIS_AMD_* switches:
- the workgroup's LDS array of per-cell sums (cellest_add / cellest_flush) at or below a cap;
- every wave's direct-mapped cache of per-cell sums (physics.h est_cache_add / est_cache_add_one: slot = cell & 127, a lane
  claims a slot, the cell that held it is flushed) above the k_rpkt / k_thermal caps;
- device-wide atomics otherwise (k_gamma above its cap, ARTIS_AMD_ESTCACHE=0, ARTIS_AMD_CELLEST_LDS=0 for k_gamma, k_rpkt with
  the line list in LDS above 512 cells -- ARTIS_AMD_LINELDS=1, whose LDS array holds at most 512 cells -- and k_thermal_q,
  ARTIS_AMD_REFILL=1; k_thermal<1024, 2> is asserted in test_gpu_parity.py's w7big case);
- the detailed bound-free estimators of the nltenebular build: k_bfest_dense with the continuum table in LDS or in HBM and
  16 / 32 / 64 lanes per record, or added in place inside k_rpkt (ARTIS_AMD_BFDEFER=0).
1D spherical grids make the non-empty cell count equal to ncoord, so that every cap is met from both sides. Every run asserts
through artis_amd_last_estimator_forms() that the form it targets ran. A lost or doubled flush of a rarely visited cell shows
as a per-entry difference of that cell however small its sums are.
"""
import numpy as np
import pytest

import parity
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-9
EST_RTOL = 1e-9
# forms of one device against each other: packets, generator states and counters identical; the estimators differ by the order
# of their float additions only (worst per-entry difference measured on the MI355X over every pair here: 5.9e-14, ffheatingestimator,
# 3073 cells without the waves' caches; printed at the end of the module)
PAIR_RTOL = 1e-12

RPKT = ("RPKT_LDS_CONT", "RPKT_LDS_NOCONT", "RPKT_LDS_LINE", "RPKT_WAVECACHE", "RPKT_GLOBAL")
THERMAL = ("THERMAL_LDS", "THERMAL_WAVECACHE", "THERMAL_GLOBAL")
GAMMA = ("GAMMA_LDS", "GAMMA_GLOBAL")
BF = ("BF_INPLACE", "BF_DENSE_CONTLDS", "BF_DENSE_HBM", "BF_LPR16", "BF_LPR32", "BF_LPR64")

# ncells -> the runs on that grid: (switches, the forms expected of k_rpkt, k_thermal, k_gamma[, forms that later, smaller
# launches of the same call may take as well]). The first run of a grid is the default; the others are compared with it as well
# as with the oracle.
CAP_RUNS = {
    512: [({}, ("RPKT_LDS_CONT", "THERMAL_LDS", "GAMMA_LDS")),
          ({"ARTIS_AMD_CELLEST_LDS": "0"}, ("RPKT_WAVECACHE", "THERMAL_WAVECACHE", "GAMMA_GLOBAL")),
          ({"ARTIS_AMD_LINELDS": "1"}, ("RPKT_LDS_LINE", "THERMAL_LDS", "GAMMA_LDS"))],
    513: [({}, ("RPKT_LDS_NOCONT", "THERMAL_LDS", "GAMMA_LDS")),
          ({"ARTIS_AMD_RPKT_EST_OVER_CONT": "0"}, ("RPKT_WAVECACHE", "THERMAL_LDS", "GAMMA_LDS"))],
    2048: [({}, ("RPKT_LDS_NOCONT", "THERMAL_LDS", "GAMMA_LDS"))],
    2049: [({}, ("RPKT_LDS_NOCONT", "THERMAL_LDS", "GAMMA_GLOBAL")),
           ({"ARTIS_AMD_CELLEST_LDS": "0"}, ("RPKT_WAVECACHE", "THERMAL_WAVECACHE", "GAMMA_GLOBAL"))],
    3072: [({}, ("RPKT_LDS_NOCONT", "THERMAL_LDS", "GAMMA_GLOBAL")),
           ({"ARTIS_AMD_RPKT_EST_OVER_CONT": "0"}, ("RPKT_WAVECACHE", "THERMAL_LDS", "GAMMA_GLOBAL"))],
    3073: [({}, ("RPKT_WAVECACHE", "THERMAL_LDS", "GAMMA_GLOBAL")),
           ({"ARTIS_AMD_ESTCACHE": "0"}, ("RPKT_GLOBAL", "THERMAL_LDS", "GAMMA_GLOBAL")),
           ({"ARTIS_AMD_RPKT_EST_OVER_CONT": "0"}, ("RPKT_WAVECACHE", "THERMAL_LDS", "GAMMA_GLOBAL")),
           # (the line list in LDS leaves no room for the waves' caches)
           ({"ARTIS_AMD_LINELDS": "1"}, ("RPKT_GLOBAL", "THERMAL_LDS", "GAMMA_GLOBAL"))],
    4096: [({}, ("RPKT_WAVECACHE", "THERMAL_LDS", "GAMMA_GLOBAL"))],
    # unsorted work lists: the 64 lanes of an instruction sit in unrelated cells, so that they contend for slots (the claim) and
    # evict one another's cells all the time, also in k_thermal, whose packets stay in their cells
    4097: [({}, ("RPKT_WAVECACHE", "THERMAL_WAVECACHE", "GAMMA_GLOBAL")),
           ({"ARTIS_AMD_ESTCACHE": "0"}, ("RPKT_GLOBAL", "THERMAL_GLOBAL", "GAMMA_GLOBAL")),
           ({"ARTIS_AMD_SORT": "0"}, ("RPKT_WAVECACHE", "THERMAL_WAVECACHE", "GAMMA_GLOBAL")),
           # k_thermal_q (lists of >= 4096 entries; shorter ones take k_thermal with its caches) adds with device-wide atomics
           ({"ARTIS_AMD_REFILL": "1"}, ("RPKT_WAVECACHE", "THERMAL_GLOBAL", "GAMMA_GLOBAL"), ("THERMAL_WAVECACHE",))],
}
PACKETS_PER_CELL = 150
CAP_PKW = dict(kpkt_fraction=0.3, gamma_fraction=0.15)

# nltenebular: the detailed bound-free estimators (bfrate_raw) and the radiation-field bins
NEB_CELLS, NEB_NPK = 64, 24000
NEB_RUNS = [({}, ("BF_DENSE_CONTLDS", "BF_LPR32")),
            ({"ARTIS_AMD_DENSE_CONTLDS": "0"}, ("BF_DENSE_HBM", "BF_LPR32")),
            ({"ARTIS_AMD_DENSE_LPR": "16"}, ("BF_DENSE_CONTLDS", "BF_LPR16")),
            ({"ARTIS_AMD_DENSE_LPR": "64"}, ("BF_DENSE_CONTLDS", "BF_LPR64")),
            ({"ARTIS_AMD_BFDEFER": "0"}, ("BF_INPLACE",))]

# the worst per-entry differences met, printed at the end of the module (the figures the bars were set against)
MEASURED = {}


def _cap_inputs(ncells):
    # (a shorter timestep on the finest grids: an r-packet there crosses ~1300 shells in the default one, and the device's libm
    # rounding, carried through that many boundary distances, takes its position beyond FLOAT_RTOL -- 2e-9 at 4096 shells;
    # ~400 crossings still fill every slot of a wave's cache several times over)
    bkw = dict(width_frac=0.015) if ncells >= 4096 else {}
    model, cs, ts, aux = synth.build("tiny", ncoord=ncells, gridtype=abi.GRID_SPHERICAL1D, **bkw)
    assert model["npts_nonempty"] == ncells
    pk0 = synth.make_packets(model, aux, PACKETS_PER_CELL * ncells, **CAP_PKW)
    return model, cs, ts, pk0


def _neb_inputs():
    model, cs, ts, aux = synth.build("small", ncoord=NEB_CELLS, gridtype=abi.GRID_SPHERICAL1D, options="nltenebular", nts=13)
    pk0 = synth.make_packets(model, aux, NEB_NPK, kpkt_fraction=0.15, gamma_fraction=0.1)
    return model, cs, ts, pk0


@pytest.fixture(scope="module")
def oracle_paths(oracle):
    """The oracle's answers, computed in forked worker processes BEFORE this process touches the GPU."""
    out = {}
    for n in CAP_RUNS:
        model, cs, ts, pk0 = _cap_inputs(n)
        pa, ea = pk0.copy(), abi.estimators_for(model)
        parity.oracle_parallel(model, cs, ts, pa, ea)
        out[n] = (model, cs, ts, pk0, pa, ea)
    model, cs, ts, pk0 = _neb_inputs()
    pa, ea = pk0.copy(), abi.estimators_for(model, "nltenebular")
    parity.oracle_parallel(model, cs, ts, pa, ea, preset="nltenebular")
    out["nltenebular"] = (model, cs, ts, pk0, pa, ea)
    return out


@pytest.fixture(scope="module")
def engine_mod(oracle_paths):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from artis_amd import engine

    engine.load_library()
    yield engine
    for k, v in sorted(MEASURED.items()):
        print(f"worst per-entry rel. difference {k}: " + ", ".join(f"{a} {w:.2e}" for a, w in sorted(v.items()) if w > 0))


def _run(engine_mod, model, cs, ts, pk0, options, switches, monkeypatch):
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    eng = None
    try:
        eng = engine_mod.Engine(model, preset=options)  # (the switches are read when the engine is made)
        eng.set_cellstate(cs, ts)
        pb, eb = pk0.copy(), abi.estimators_for(model, options)
        eng.update_packets(pb, eb)
        forms, variants = eng.last_estimator_forms(), eng.last_thermal_variants()
    finally:
        if eng is not None:
            eng.close()
        for k in switches:
            monkeypatch.delenv(k, raising=False)
    return pb, eb, forms, variants


def _family(forms, names):
    return {k for k in names if forms & abi.EST_FORMS[k]}


def _check(tag, pb, eb, pa, ea, base):
    parity.compare_packets(pb, pa, FLOAT_RTOL, f"{tag}: HIP engine vs oracle")
    parity.compare_stats(eb, ea, f"{tag}: HIP engine vs oracle", same_libm=False)
    MEASURED[f"{tag} vs oracle"] = parity.compare_estimators(eb, ea, EST_RTOL, f"{tag}: HIP engine vs oracle")
    if base is not None:  # the default form of the same grid on the same device
        p0, e0 = base
        parity.compare_packets(pb, p0, 0.0, f"{tag}: vs the default form")
        parity.compare_stats(eb, e0, f"{tag}: vs the default form")
        MEASURED[f"{tag} vs default"] = parity.compare_estimators(eb, e0, PAIR_RTOL, f"{tag}: vs the default form")


@pytest.mark.parametrize("ncells", sorted(CAP_RUNS))
def test_cell_estimator_paths_at_caps_match_oracle(engine_mod, oracle_paths, monkeypatch, ncells):
    model, cs, ts, pk0, pa, ea = oracle_paths[ncells]
    # the regime the caches were built for: ~100 packets start in most cells, and an r-packet crosses more cells than a wave's
    # cache has slots (1D shells: consecutive cells take consecutive slots, so a wave's packets evict). This is shown on the oracle's
    # side only, by the mean cell crossings per packet -- crossings, not distinct cells per wave; the device counts no evictions.
    # (k_thermal's packets stay in their cells: its slots contend in the unsorted-list run, where a wave's lanes sit in unrelated
    # cells.)
    starts = np.bincount(pk0["cellindex"], minlength=ncells)
    assert np.median(starts) >= 100, np.median(starts)
    st = ea.stats_dict()
    assert st["CELLCROSSINGS"] > 128 * len(pk0), st["CELLCROSSINGS"] / len(pk0)
    assert ea.colheatingestimator.sum() > 0 and ea.dep_estimator_gamma.sum() > 0 and st["X_GAMMA_STEPS"] > 0
    base = None
    for switches, want, *also in CAP_RUNS[ncells]:
        tag = f"{ncells} cells {switches or 'default'}"
        pb, eb, forms, variants = _run(engine_mod, model, cs, ts, pk0, "classic", switches, monkeypatch)
        got = _family(forms, RPKT) | _family(forms, THERMAL) | _family(forms, GAMMA)
        assert set(want) <= got <= set(want) | set(*also), f"{tag}: estimator forms {sorted(got)} ({forms:#x}), expected {sorted(want)}"
        if "ARTIS_AMD_REFILL" in switches:
            assert variants & engine_mod.Engine.THERMAL_REFILL, f"{tag}: k_thermal_q did not run ({variants:#x})"
        _check(tag, pb, eb, pa, ea, base)
        if base is None:
            base = (pb, eb)


def test_bound_free_estimator_paths_match_oracle(engine_mod, oracle_paths, monkeypatch):
    model, cs, ts, pk0, pa, ea = oracle_paths["nltenebular"]
    assert np.count_nonzero(ea.bfrate_raw) > 2000 and np.count_nonzero(ea.radfieldbin_J) > 2000
    base = None
    for switches, want in NEB_RUNS:
        tag = f"nltenebular {switches or 'default'}"
        pb, eb, forms, _ = _run(engine_mod, model, cs, ts, pk0, "nltenebular", switches, monkeypatch)
        got = _family(forms, BF)
        assert got == set(want), f"{tag}: bound-free estimator forms {sorted(got)} ({forms:#x}), expected {sorted(want)}"
        _check(tag, pb, eb, pa, ea, base)
        if base is None:
            base = (pb, eb)
