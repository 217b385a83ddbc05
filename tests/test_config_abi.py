"""CPU-side checks of the engine configuration in the C-ABI (include/artis_amd.h artis_amd_config / artis_amd_plan): the ctypes mirrors
against the C compiler's layout and the library's own sizes, the defaults, the configuration's validation -- which runs before the device
is touched, so it is tested here -- and artis_amd_engine_plan with a given free memory, which needs no device either."""
import ctypes as C
import os
import subprocess

import pytest

from artis_amd import abi, engine, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ERR_ARG = -3
FREE = 10 << 30  # a free memory handed to the plan: the device is not asked


@pytest.fixture(scope="module")
def lib():
    return engine.load_library(build_if_missing=True)


@pytest.fixture(scope="module")
def small5():
    """the smallest synthetic model of the tiling tests: the 5^3 grid (81 non-empty cells)"""
    return synth.build("small", ncoord=5)[0]


def test_ctypes_mirrors_match_the_header_and_the_library(lib, tmp_path):
    exe = str(tmp_path / "config_printer")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "config_printer.c")])
    got = {}
    for line in subprocess.check_output([exe], text=True).strip().splitlines():
        name, offset, size = line.split()
        got[name] = (int(offset), int(size))
    for prefix, cls, libsize in (("config", abi.Config, lib.artis_amd_sizeof_config()), ("plan", abi.Plan, lib.artis_amd_sizeof_plan())):
        assert C.sizeof(cls) == got.pop(f"{prefix}.sizeof")[0] == libsize, prefix
        fields = {k: v for k, v in got.items() if k.startswith(prefix + ".")}
        assert [k.split(".")[1] for k in fields] == [n for n, _ in cls._fields_], prefix  # the same fields in the same order
        for name, _ in cls._fields_:
            d = getattr(cls, name)
            assert (d.offset, d.size) == fields[f"{prefix}.{name}"], (prefix, name)


def test_config_default_sets_every_sentinel(lib):
    cfg = abi.Config()
    C.memset(C.byref(cfg), 0x5A, C.sizeof(cfg))
    lib.artis_amd_config_default(C.byref(cfg))
    assert cfg.struct_size == C.sizeof(abi.Config) == lib.artis_amd_sizeof_config()
    assert {k: v for k, v in abi.struct_dict(cfg).items() if k != "struct_size"} == abi.CONFIG_DEFAULTS
    assert abi.struct_dict(abi.config()) == abi.struct_dict(cfg)  # the Python-side constructor gives the same struct


@pytest.mark.parametrize("fields,word", [(dict(struct_size=C.sizeof(abi.Config) + 8), "struct_size"), (dict(reserved=1), "reserved"),
                                         (dict(ma_hot_fraction=0.0), "ma_hot_fraction"), (dict(ma_hot_fraction=1.5), "ma_hot_fraction"),
                                         (dict(ma_pool_fraction=-0.5), "ma_pool_fraction"), (dict(keep_line_dpop=2), "keep_line_dpop"),
                                         (dict(cache_budget_bytes=-5), "cache_budget_bytes"), (dict(tile_park_at=-2), "tile_park_at")])
def test_create_ex_refuses_a_bad_config_before_it_touches_the_device(lib, small5, fields, word):
    """ARTIS_ERR_ARG with the field's name in artis_amd_last_error(), with or without a device: a missing device would be ARTIS_ERR_NODEVICE"""
    cfg = abi.config()
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = C.c_void_p(0xDEAD)
    rc = lib.artis_amd_engine_create_ex(C.cast(small5.ref(), C.c_void_p), 0, C.byref(cfg), C.byref(h))
    msg = lib.artis_amd_last_error().decode()
    assert rc == ERR_ARG and h.value is None, (rc, h.value, msg)
    assert msg and word in msg, msg
    plan = abi.Plan(struct_size=C.sizeof(abi.Plan))
    assert lib.artis_amd_engine_plan(C.cast(small5.ref(), C.c_void_p), 0, C.byref(cfg), FREE, C.byref(plan)) == ERR_ARG


def test_smaller_struct_size_of_an_older_caller_is_accepted(lib, small5):
    """A struct that ends after ma_hot_fraction: the fields it has count, the bytes beyond it are not read (they hold what would be refused)."""
    n = small5["npts_nonempty"]
    full = engine.plan(small5, dict(ma_hot_fraction=0.5), free_bytes=FREE)
    cfg = abi.config(ma_hot_fraction=0.5, ma_pool_fraction=-7.0, keep_line_dpop=9, reserved=1)
    cfg.struct_size = abi.Config.ma_pool_fraction.offset
    assert engine.plan(small5, cfg, free_bytes=FREE) == full
    assert full["hot_fraction"] == 0.5 and full["ncold_levels"] > 0 and full["cells_resident"] == n


def test_plan_with_given_budget_and_free_memory_needs_no_device(small5):
    n = small5["npts_nonempty"]
    whole = engine.plan(small5, free_bytes=FREE)
    assert whole["ntiles"] == 1 and whole["cells_resident"] == n and whole["hot_fraction"] == 1.0 and whole["line_dpop_kept"] == 1
    assert whole["free_bytes_assumed"] == FREE and whole["ncold_levels"] == 0 and whole["pool_slots"] == 0
    assert whole["cache_bytes"] >= n * whole["bytes_per_cell"] and whole["model_bytes"] > 0 and whole["pop_scratch_bytes"] > 0
    # a quarter of the whole cache, static records: rows that fit = budget // row, tiles = ceil(cells / rows)
    budget = n * whole["bytes_per_cell"] // 4
    q = engine.plan(small5, dict(cache_budget_bytes=budget, ma_hot_fraction=1.0), free_bytes=FREE)
    fit = budget // q["bytes_per_cell"]
    assert q["cells_resident"] == fit and q["ntiles"] == -(-n // fit) and q["ntiles"] in (4, 5), q
    assert q["cells_resident"] * q["ntiles"] >= n
    assert q["line_dpop_kept"] == 0 and q["bytes_per_cell"] == whole["bytes_per_cell"] - 8 * small5["nlines"]  # dropped: it saves a tile
    # ... and a pure function of model and config: another free memory changes nothing but the echo of it
    q2 = engine.plan(small5, dict(cache_budget_bytes=budget, ma_hot_fraction=1.0), free_bytes=20 * FREE)
    assert {**q2, "free_bytes_assumed": FREE} == q
    # the automatic rule does depend on it: 80 % of what is free less the 2 GB scratch cannot hold the cache when 2 GB and 1 MB are free
    tight = engine.plan(small5, free_bytes=(2 << 30) + (1 << 20) + whole["model_bytes"])
    assert tight["ntiles"] > 1 and tight["free_bytes_assumed"] == (2 << 30) + (1 << 20) + whole["model_bytes"]


def test_plan_refuses_budgets_that_hold_no_row(small5):
    whole = engine.plan(small5, free_bytes=FREE)
    row, slim = whole["bytes_per_cell"], whole["bytes_per_cell"] - 8 * small5["nlines"]
    with pytest.raises(engine.EngineError, match="cannot hold one row"):
        engine.plan(small5, dict(cache_budget_bytes=slim - 1, ma_hot_fraction=1.0), free_bytes=FREE)
    # between the row without line_dpop and the row with it: fine for rows without it, refused when the rows have to keep it
    ok = engine.plan(small5, dict(cache_budget_bytes=row - 1, ma_hot_fraction=1.0, keep_line_dpop=0), free_bytes=FREE)
    assert ok["cells_resident"] == 1 and ok["line_dpop_kept"] == 0 and ok["ntiles"] == small5["npts_nonempty"]
    with pytest.raises(engine.EngineError, match="keep_line_dpop"):
        engine.plan(small5, dict(cache_budget_bytes=row - 1, ma_hot_fraction=1.0, keep_line_dpop=1), free_bytes=FREE)


def test_plan_takes_the_variables_where_the_struct_leaves_a_field_alone(small5, monkeypatch):
    """precedence, on the CPU: struct field, else ARTIS_AMD_* variable, else default"""
    n = small5["npts_nonempty"]
    for k in ("ARTIS_AMD_CACHE_BUDGET_MB", "ARTIS_AMD_MA_HOTFRAC", "ARTIS_AMD_MA_POOLFRAC", "ARTIS_AMD_DPOP", "ARTIS_AMD_POP_SCRATCH_MB"):
        monkeypatch.delenv(k, raising=False)
    whole = engine.plan(small5, free_bytes=FREE)
    third = (n // 3 + 1) * whole["bytes_per_cell"]
    monkeypatch.setenv("ARTIS_AMD_CACHE_BUDGET_MB", repr(third / 1048576.0))
    monkeypatch.setenv("ARTIS_AMD_MA_HOTFRAC", "1")
    from_env = engine.plan(small5, free_bytes=FREE)
    assert from_env["ntiles"] == 3 and from_env["hot_fraction"] == 1.0
    assert engine.plan(small5, dict(cache_budget_bytes=third, ma_hot_fraction=1.0), free_bytes=FREE) == from_env
    over = engine.plan(small5, dict(cache_budget_bytes=2 * n * whole["bytes_per_cell"], ma_hot_fraction=0.3, ma_pool_fraction=1.0), free_bytes=FREE)
    assert over["ntiles"] == 1 and over["hot_fraction"] == 0.3 and over["ncold_levels"] > 0 and over["pool_slots"] > 0
    monkeypatch.setenv("ARTIS_AMD_MA_HOTFRAC", "0.3")
    monkeypatch.setenv("ARTIS_AMD_MA_POOLFRAC", "1")
    assert engine.plan(small5, dict(cache_budget_bytes=2 * n * whole["bytes_per_cell"]), free_bytes=FREE) == over


def test_abi_version_is_unchanged(lib):
    assert lib.artis_amd_abi_version() == abi.ABI_VERSION == 6
