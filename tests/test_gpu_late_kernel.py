"""GPU tests of k_late: one persistent launch that carries the r-packets and thermal packets of the end of a population
through all their r-packet <-> thermal alternations, by wave role, on per-workgroup queues. Where a packet is advanced is placement: every
field of every packet, the generator states and the event counters are those of the split kernels; the estimators are theirs to summation
order. Every run sets ARTIS_AMD_LATE_STRICT=1, which turns a wave of k_late that gave up waiting for work into an error.

Shapes: the tail kernel's test's (tests/test_gpu_parity.py) -- the `small` atomic data on 8^3, 16 shells and the kilonova_lte options, 30 000
packets of every type so that packets leave k_late for every other kernel and come back; the bench's atomic data (`w7`: tables of the size the
headline puts into k_late's LDS) on 136 cells; and the edges of the partition into one share per workgroup."""
import numpy as np
import pytest

import parity
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-9  # packets against the oracle (test_gpu_parity.FLOAT_RTOL)
LATE_VARIABLES = ("ARTIS_AMD_LATE", "ARTIS_AMD_LATE_ALWAYS", "ARTIS_AMD_LATE_STRICT")
NEVER = {"ARTIS_AMD_LATE": "0"}
ALWAYS = {"ARTIS_AMD_LATE": "100000000", "ARTIS_AMD_LATE_ALWAYS": "1"}


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from artis_amd import engine

    engine.load_library()
    return engine


def run(engine_mod, monkeypatch, model, cs, ts, pk0, env, options="classic", config=None):
    """one step of the packets on a new engine created under `env` (+ ARTIS_AMD_LATE_STRICT=1)"""
    for v in LATE_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ARTIS_AMD_LATE_STRICT", "1")
    eng = engine_mod.Engine(model, preset=options, config=config)
    tiles = eng.cache_tiles()
    eng.set_cellstate(cs, ts)
    p, e = pk0.copy(), abi.estimators_for(model, options)
    eng.update_packets(p, e)
    out = dict(p=p, e=e, late_ms=eng.last_kernel_ms_by_kind()["k_late"]["ms"], variants=eng.last_thermal_variants(), tiles=tiles)
    eng.close()
    return out


def ran_late(engine_mod, out):
    bit = bool(out["variants"] & engine_mod.Engine.THERMAL_LATE)
    assert bit == (out["late_ms"] > 0), (out["variants"], out["late_ms"])
    return bit


def same(got, want, what):
    parity.compare_packets(got["p"], want["p"], 0.0, what)
    assert np.array_equal(got["p"]["rngstate"], want["p"]["rngstate"]), what
    parity.compare_stats(got["e"], want["e"], what)
    parity.compare_estimators(got["e"], want["e"], 1e-11, what)


@pytest.mark.parametrize("options,gridtype,ncoord", [("classic", abi.GRID_CARTESIAN3D, 8), ("classic", abi.GRID_SPHERICAL1D, 16),
                                                     ("kilonova_lte", abi.GRID_CARTESIAN3D, 8)])
def test_late_kernel_gives_the_split_kernels_packets(engine_mod, oracle, monkeypatch, options, gridtype, ncoord):
    """Never (ARTIS_AMD_LATE=0), the whole population from its first visit (ARTIS_AMD_LATE_ALWAYS), the end of a population that began above
    the threshold (ARTIS_AMD_LATE=8000) and the default (30 000 packets begin below it): identical packets and counters, estimators to
    summation order; the oracle's packets; and k_late ran exactly where it was meant to."""
    model, cs, ts, aux = synth.build("small", ncoord=ncoord, gridtype=gridtype, options=options)
    pk0 = synth.make_packets(model, aux, 30000, kpkt_fraction=0.2, gamma_fraction=0.1, pellet_fraction=0.1)
    outs = [run(engine_mod, monkeypatch, model, cs, ts, pk0, env, options) for env in (NEVER, ALWAYS, {"ARTIS_AMD_LATE": "8000"}, {})]
    assert [ran_late(engine_mod, o) for o in outs] == [False, True, True, False]
    for o in outs[1:]:
        same(o, outs[0], "k_late vs split kernels")
    pa, ea = pk0[:6000].copy(), abi.estimators_for(model, options)
    oracle.update_packets(model, cs, ts, pa, ea, preset=options)
    parity.compare_packets(outs[1]["p"][:6000], pa, FLOAT_RTOL, "k_late vs oracle")


def test_late_kernel_with_the_bench_tables_in_lds(engine_mod, oracle, monkeypatch):
    """the bench's atomic data (1567 levels, 27 238 transitions, the continuum table: what the headline stages in k_late's LDS) on 136 cells,
    mostly k-packets"""
    model, cs, ts, aux = synth.build("w7", ncoord=6)
    pk0 = synth.make_packets(model, aux, 6000, kpkt_fraction=0.8)
    never = run(engine_mod, monkeypatch, model, cs, ts, pk0, NEVER)
    always = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALWAYS)
    assert not ran_late(engine_mod, never) and ran_late(engine_mod, always)
    same(always, never, "k_late (bench tables) vs split kernels")
    pa, ea = pk0.copy(), abi.estimators_for(model, "classic")
    oracle.update_packets(model, cs, ts, pa, ea)
    parity.compare_packets(always["p"], pa, FLOAT_RTOL, "k_late (bench tables) vs oracle")


@pytest.mark.parametrize("npk", [100, 257 * 64 + 1])
def test_late_kernel_partition_edges(engine_mod, monkeypatch, npk):
    """fewer packets than workgroups (most queues begin empty), and one packet more than a whole number of waves"""
    model, cs, ts, aux = synth.build("small", ncoord=8)
    pk0 = synth.make_packets(model, aux, npk, kpkt_fraction=0.2, gamma_fraction=0.1, pellet_fraction=0.1)
    never = run(engine_mod, monkeypatch, model, cs, ts, pk0, NEVER)
    always = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALWAYS)
    assert not ran_late(engine_mod, never) and ran_late(engine_mod, always)
    same(always, never, f"k_late vs split kernels, {npk} packets")


def test_late_kernel_is_not_used_where_it_is_not_eligible(engine_mod, monkeypatch):
    """a tiled cache, and a build with virtual packets: ARTIS_AMD_LATE_ALWAYS changes nothing"""
    model, cs, ts, aux = synth.build("small", ncoord=6)
    pk0 = synth.make_packets(model, aux, 6000, kpkt_fraction=0.2)
    base = run(engine_mod, monkeypatch, model, cs, ts, pk0, {})
    assert base["tiles"][0] == 1
    two = dict(cache_budget_bytes=int(base["tiles"][2]) * (model["npts_nonempty"] // 2 + 1) + 4096, ma_hot_fraction=1.0, ma_pool_fraction=1.0)
    tiled_default = run(engine_mod, monkeypatch, model, cs, ts, pk0, {}, config=two)
    tiled = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALWAYS, config=two)
    assert tiled["tiles"][0] == 2 and not ran_late(engine_mod, tiled) and not ran_late(engine_mod, tiled_default)
    same(tiled, tiled_default, "tiled engine, ARTIS_AMD_LATE_ALWAYS vs default")
    P = "ci_classic_vpkt"
    vmodel, vcs, vts, vaux = synth.build("small", ncoord=5, options=P, t_days=5.0)
    vpk0 = synth.make_packets(vmodel, vaux, 6000, kpkt_fraction=0.2)
    vbase = run(engine_mod, monkeypatch, vmodel, vcs, vts, vpk0, {}, options=P)
    valways = run(engine_mod, monkeypatch, vmodel, vcs, vts, vpk0, ALWAYS, options=P)
    assert not ran_late(engine_mod, vbase) and not ran_late(engine_mod, valways)
    same(valways, vbase, "virtual-packet build, ARTIS_AMD_LATE_ALWAYS vs default")
