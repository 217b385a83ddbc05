"""GPU tests of the engine configuration in the C-ABI (include/artis_amd.h artis_amd_config, artis_amd_engine_create_ex, artis_amd_engine_config,
artis_amd_engine_plan): a field set in the struct does what its ARTIS_AMD_* variable does, and wins over it; two engines of one process take two
configurations; the plan is the layout the engine then builds; what the struct cannot have is refused and leaves nothing behind.

Shapes: the tiling tests' (tests/test_gpu_parity.py) at their smallest -- the `small` atomic data on the 6^3 grid (136 non-empty cells), 6000
packets (above the tail kernel's default threshold of 4096, so that a default run does launch it), a budget of a third of the static rows.
The on-demand case is that model with 0.3 of every ion's levels hot, as test_cell_cache_tiling_gives_identical_packets has it: building the
large on-demand data set alone takes 25 s of host time. Every engine here sees the same packets; the default run is made once and shared."""
import ctypes as C

import numpy as np
import pytest

import parity
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-9  # packets against the oracle (test_gpu_parity.FLOAT_RTOL)
EST_RTOL = 1e-9    # estimators of a tiled against an untiled run (test_gpu_parity.EST_RTOL; tests/parity.py holds the comparison, not the number)
ERR_ARG, ERR_UNSUPPORTED = -3, -4
UPDATECELL = abi.STAT_NAMES.index("UPDATECELL")
CONFIG_VARIABLES = ("ARTIS_AMD_CACHE_BUDGET_MB", "ARTIS_AMD_CACHE_HEADROOM_MB", "ARTIS_AMD_POP_SCRATCH_MB", "ARTIS_AMD_MA_HOTFRAC",
                    "ARTIS_AMD_MA_POOLFRAC", "ARTIS_AMD_TAIL", "ARTIS_AMD_TAIL_ALWAYS", "ARTIS_AMD_TILE_PARK", "ARTIS_AMD_TILE_PARK_AT", "ARTIS_AMD_DPOP")


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from artis_amd import engine

    engine.load_library()
    return engine


@pytest.fixture(autouse=True)
def no_config_variables(monkeypatch):
    """the caller's environment configures nothing here: a test sets what it means to set"""
    for k in CONFIG_VARIABLES:
        monkeypatch.delenv(k, raising=False)


def run(engine_mod, case, config=None, engine=None):
    """one step of the case's packets on a new engine (or on `engine`, which stays open): everything a test compares"""
    model, cs, ts, pk0 = case["model"], case["cs"], case["ts"], case["pk0"]
    eng = engine or engine_mod.Engine(model, config=config)
    out = dict(tiles=eng.cache_tiles(), tiers=eng.record_tiers(), config=eng.config())
    eng.set_cellstate(cs, ts)
    p, est = pk0.copy(), abi.estimators_for(model, "classic")
    eng.update_packets(p, est)
    out.update(p=p, est=est, tiling=eng.last_tiling(), kinds=eng.last_kernel_ms_by_kind(), variants=eng.last_thermal_variants())
    if engine is None:
        eng.close()
    return out


def same_packets(got, want, what, layout_differs=False):
    """packets, generator states and counters bit for bit (a run with another layout fills cells more often: UPDATECELL); estimators to EST_RTOL"""
    parity.compare_packets(got["p"], want["p"], 0.0, what)
    assert np.array_equal(got["p"]["rngstate"], want["p"]["rngstate"]), what
    mask = np.arange(abi.NSTATS) != (UPDATECELL if layout_differs else -1)
    assert np.array_equal(got["est"].stats[mask], want["est"].stats[mask]), what
    parity.compare_estimators(got["est"], want["est"], EST_RTOL, what)


@pytest.fixture(scope="module")
def case(engine_mod):
    """model, cell state, packets, the default engine's run (no variable set, no struct) and the budget of a third of its rows"""
    import os

    saved = {k: os.environ.pop(k) for k in CONFIG_VARIABLES if k in os.environ}
    try:
        model, cs, ts, aux = synth.build("small", ncoord=6)
        c = dict(model=model, cs=cs, ts=ts, pk0=synth.make_packets(model, aux, 6000, kpkt_fraction=0.2), n=model["npts_nonempty"])
        c["base"] = run(engine_mod, c)
    finally:
        os.environ.update(saved)
    assert c["base"]["tiles"][0] == 1 and c["base"]["tiers"]["ncold"] == 0
    c["third"] = int(c["base"]["tiles"][2]) * (c["n"] // 3 + 1) + 4096  # [B] a third of the cells' static rows
    return c


def three_tiles(case):
    return dict(cache_budget_bytes=case["third"], ma_hot_fraction=1.0, ma_pool_fraction=1.0)


def on_demand(case):
    return dict(cache_budget_bytes=case["third"], ma_hot_fraction=0.3, ma_pool_fraction=1.0)


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["three_static_tiles", "on_demand_records"])
def test_struct_equals_environment(engine_mod, case, monkeypatch, which):
    cfg = three_tiles(case) if which == "three_static_tiles" else on_demand(case)
    by_struct = run(engine_mod, case, config=cfg)
    monkeypatch.setenv("ARTIS_AMD_CACHE_BUDGET_MB", repr(cfg["cache_budget_bytes"] / 1048576.0))  # (an integer below 2^53 over 2^20: exact both ways)
    monkeypatch.setenv("ARTIS_AMD_MA_HOTFRAC", repr(cfg["ma_hot_fraction"]))
    monkeypatch.setenv("ARTIS_AMD_MA_POOLFRAC", repr(cfg["ma_pool_fraction"]))
    by_env = run(engine_mod, case)  # artis_amd_engine_create, as every caller before the struct
    for k in ("tiles", "tiers", "config"):
        assert by_struct[k] == by_env[k], (k, by_struct[k], by_env[k])
    same_packets(by_struct, by_env, f"{which}: struct vs environment")
    assert by_struct["config"]["cache_budget_bytes"] == cfg["cache_budget_bytes"] and by_struct["config"]["ma_pool_fraction"] == 1.0
    if which == "three_static_tiles":
        assert by_struct["tiles"][0] == 3 and by_struct["tiers"]["ncold"] == 0, by_struct["tiles"]
    else:
        assert by_struct["tiers"]["hot_fraction"] == 0.3 and by_struct["tiers"]["ncold"] > 0 and by_struct["tiers"]["pool_slots"] > 0
        assert by_struct["variants"] & engine_mod.Engine.THERMAL_COLD, by_struct["variants"]  # the on-demand look-ups ran
    same_packets(by_struct, case["base"], f"{which}: struct vs default engine", layout_differs=True)


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
def test_struct_field_wins_over_its_variable(engine_mod, case, monkeypatch):
    monkeypatch.setenv("ARTIS_AMD_CACHE_BUDGET_MB", "64")  # the whole cache several times over: one tile
    monkeypatch.setenv("ARTIS_AMD_MA_HOTFRAC", "1")
    monkeypatch.setenv("ARTIS_AMD_TAIL", "777")
    eng = engine_mod.Engine(case["model"], config=dict(cache_budget_bytes=case["third"], tail_threshold=1234))
    assert eng.cache_tiles()[0] == 3
    got = eng.config()
    eng.close()
    assert got["cache_budget_bytes"] == case["third"] and got["tail_threshold"] == 1234 and got["ma_hot_fraction"] == 1.0
    # the struct's fields at "automatic": the variables' values come back
    eng = engine_mod.Engine(case["model"], config=abi.config())
    assert eng.cache_tiles()[0] == 1
    got = eng.config()
    eng.close()
    assert got["cache_budget_bytes"] == 64 * 1048576 and got["tail_threshold"] == 777 and got["ma_hot_fraction"] == 1.0
    # ... and with neither, the defaults, every "automatic" resolved
    for k in ("ARTIS_AMD_CACHE_BUDGET_MB", "ARTIS_AMD_MA_HOTFRAC", "ARTIS_AMD_TAIL"):
        monkeypatch.delenv(k)
    got = case["base"]["config"]
    assert got["tail_threshold"] == 4096 and got["tile_park_at"] == 3145728 and got["pop_scratch_bytes"] == 2048 << 20
    assert got["cache_headroom_bytes"] == 0 and got["ma_pool_fraction"] == 0.15 and got["keep_line_dpop"] == 1 and got["reserved"] == 0
    assert got["cache_budget_bytes"] > case["n"] * case["base"]["tiles"][2]  # what the automatic rule made of the free memory


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_engines_of_one_process_take_two_configurations(engine_mod, case):
    whole = engine_mod.Engine(case["model"], config=dict(ma_hot_fraction=1.0))
    tiled = engine_mod.Engine(case["model"], config=three_tiles(case))
    try:
        assert whole.cache_tiles()[0] == 1 and tiled.cache_tiles()[0] == 3
        a = run(engine_mod, case, engine=whole)
        b = run(engine_mod, case, engine=tiled)
        assert whole.cache_tiles()[0] == 1 and tiled.cache_tiles()[0] == 3  # (still: each engine kept its own)
    finally:
        whole.close()
        tiled.close()
    assert b["tiling"]["tile_fills"] > 0 and a["tiling"]["tile_fills"] == 0
    same_packets(b, a, "3 tiles vs untiled, two engines alive together", layout_differs=True)
    same_packets(a, case["base"], "untiled by struct vs default engine")


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default", "three_static_tiles", "on_demand_records"])
def test_plan_equals_the_engine_created_next(engine_mod, case, which):
    cfg = {"default": None, "three_static_tiles": three_tiles(case), "on_demand_records": on_demand(case)}[which]
    plan = engine_mod.plan(case["model"], cfg, free_bytes=0)
    eng = engine_mod.Engine(case["model"], config=cfg if cfg is not None else abi.config())
    tiles, tiers, eff = eng.cache_tiles(), eng.record_tiers(), eng.config()
    eng.close()
    assert (plan["ntiles"], plan["cells_resident"], plan["bytes_per_cell"]) == tiles, (plan, tiles)
    assert (plan["hot_fraction"], plan["ncold_levels"], plan["pool_slots"]) == (tiers["hot_fraction"], tiers["ncold"], tiers["pool_slots"]), (plan, tiers)
    assert plan["line_dpop_kept"] == eff["keep_line_dpop"] and plan["hot_fraction"] == eff["ma_hot_fraction"], (plan, eff)
    assert plan["free_bytes_assumed"] > 0 and plan["cache_bytes"] >= plan["cells_resident"] * plan["bytes_per_cell"]
    if cfg is not None:  # a given budget: the free memory is not part of the answer
        p10, p200 = (engine_mod.plan(case["model"], cfg, free_bytes=gb << 30) for gb in (10, 200))
        assert p10["free_bytes_assumed"] == 10 << 30 and p200["free_bytes_assumed"] == 200 << 30
        assert {**p10, "free_bytes_assumed": 0} == {**p200, "free_bytes_assumed": 0} == {**plan, "free_bytes_assumed": 0}


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_struct_leave_nothing_behind(engine_mod, case, oracle):
    L = engine_mod.load_library()
    row = case["base"]["tiles"][2]  # (with line_dpop: the default engine keeps it)
    assert case["base"]["config"]["keep_line_dpop"] == 1

    def create(lib, model, **fields):
        h, cfg = C.c_void_p(0xDEAD), abi.config(**fields)
        rc = lib.artis_amd_engine_create_ex(C.cast(model.ref(), C.c_void_p), 0, C.byref(cfg), C.byref(h))
        return rc, h.value, lib.artis_amd_last_error().decode()

    # line_dpop asked for in a budget below a row that has it (a row without it would fit)
    rc, h, msg = create(L, case["model"], cache_budget_bytes=row - 1, ma_hot_fraction=1.0, keep_line_dpop=1)
    assert rc == ERR_ARG and h is None and "keep_line_dpop" in msg, (rc, h, msg)
    # a budget that holds no row at all
    rc, h, msg = create(L, case["model"], cache_budget_bytes=1000, ma_hot_fraction=1.0)
    assert rc == ERR_ARG and h is None and "cannot hold one row" in msg, (rc, h, msg)
    # a VPKT_ON build whose cache would be tiled: today's refusal, reached through the struct
    vmodel = synth.build("small", ncoord=5, options="ci_classic_vpkt", t_days=5.0)[0]
    vplan = engine_mod.plan(vmodel, preset="ci_classic_vpkt", free_bytes=10 << 30)
    LV = engine_mod.load_library(preset="ci_classic_vpkt")
    rc, h, msg = create(LV, vmodel, cache_budget_bytes=vplan["bytes_per_cell"] * (vmodel["npts_nonempty"] // 3 + 1), ma_hot_fraction=1.0)
    assert rc == ERR_UNSUPPORTED and h is None and "VPKT_ON" in msg, (rc, h, msg)
    with pytest.raises(engine_mod.EngineError, match="VPKT_ON"):
        engine_mod.plan(vmodel, dict(cache_budget_bytes=vplan["bytes_per_cell"] * (vmodel["npts_nonempty"] // 3 + 1), ma_hot_fraction=1.0),
                        preset="ci_classic_vpkt", free_bytes=10 << 30)
    # the device is as it was: an engine created now gives the default run's packets, which are the oracle's
    after = run(engine_mod, case, config=three_tiles(case))
    same_packets(after, case["base"], "engine created after refused creations vs default engine", layout_differs=True)
    pa, ea = case["pk0"][:1500].copy(), abi.estimators_for(case["model"], "classic")
    oracle.update_packets(case["model"], case["cs"], case["ts"], pa, ea)
    parity.compare_packets(after["p"][:1500], pa, FLOAT_RTOL, "engine created after refused creations vs oracle")


# 6 ---------------------------------------------------------------------------------------------------------------------------------------
def test_tail_threshold_and_tile_park_at_take_effect(engine_mod, case):
    """budgets and thresholds place work, they change no packet"""
    base = case["base"]
    # (artis_amd_last_kernel_ms_by_kind counts no launches for k_tail: its summed duration is what shows one)
    assert base["kinds"]["k_tail"]["ms"] > 0 and base["variants"] & engine_mod.Engine.THERMAL_TAIL  # 6000 packets: the default run ends in k_tail
    never = run(engine_mod, case, config=dict(tail_threshold=0))
    assert never["kinds"]["k_tail"]["ms"] == 0 and not never["variants"] & engine_mod.Engine.THERMAL_TAIL, never["kinds"]
    assert never["config"]["tail_threshold"] == 0
    same_packets(never, base, "tail_threshold = 0 vs default")
    # three tiles, no tail kernel: nothing parks at the default tile_park_at (3145728 packets: no visit begins larger); at 200 visits park their last packets
    unparked = run(engine_mod, case, config=dict(tail_threshold=0, **three_tiles(case)))
    parked = run(engine_mod, case, config=dict(tail_threshold=0, tile_park_at=200, **three_tiles(case)))
    assert unparked["tiles"][0] == parked["tiles"][0] == 3 and parked["config"]["tile_park_at"] == 200
    assert unparked["tiling"]["parked"] == 0 and parked["tiling"]["parked"] > 0, (unparked["tiling"], parked["tiling"])
    same_packets(parked, unparked, "tile_park_at = 200 vs default", layout_differs=True)
    same_packets(parked, base, "tile_park_at = 200, 3 tiles vs default engine", layout_differs=True)
