"""GPU tests of the cell cache's population (cellcache_kernels.h, stage_cellcache.h): every array of a cell's row -- the reference's spans
(artis_amd_debug_cellcache) and what the row keeps beside them, the engine's own expansion-opacity tables and the derived non-thermal arrays
(artis_amd_debug_cellcache_array) -- against the oracle, in every build whose options change a body of the population, in every non-empty
cell, in cells whose state is an edge, and at the shapes whose loops `small` on a whole cache never takes: more than 4096 continua (a second
trip of k_keptlist over the bitmap words), 3 continua (less than a wave), more than 16 items for the 16-lane groups, a fill in several
batches, and a tiled cache whose rows are not the cells' indices. The cases and the comparison are cellcache_common.py's, shared with the
host emulation's tests (tests/test_cellcache_rules.py, bit for bit).

Bars (cellcache_common.check_against_oracle): float64 arrays 1e-12 relative, the bar of test_cellcache_matches_oracle; line_dpop -- a
difference of two nearly equal terms -- against the larger term; float32 expansionopacities one unit in the last place; integers, bitmaps and
the cooling guides exact; a tiled engine's rows against the untiled engine's byte for byte."""
import numpy as np
import pytest

import cellcache_common as cc
import hostemu_binding as emu
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from artis_amd import engine

    engine.load_library()
    return engine


def _compare_cells(eng, oracle, model, cs, ts, options, what, cells):
    worst = {}
    try:
        for c in cells:
            row = cc.view_row(eng, c, options)
            ref = cc.oracle_row(oracle, model, cs, ts, c, options)
            cc.check_against_oracle(row, ref, model, cs, c, options, False, f"{what} cell {c}", worst)
            cc.check_derived(row, model, emu.cool_guide_row, f"{what} cell {c}")
    finally:
        print(f"{what}: worst relative difference per array " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    return worst


@pytest.mark.parametrize("options", cc.BUILDS)
def test_every_array_of_every_cell_matches_oracle(engine_mod, oracle, options):
    """`small` on 4^3 cells (the innermost thick in the expansion builds: no tables for those) and, for one build, on 6 shells; every
    non-empty cell, every array, both entry points"""
    model, cs, ts, aux = synth.build("small", ncoord=4, thick_below_v=cc.THICK_BELOW_V if "expopac" in options else 0.0, options=options)
    n = int(model["npts_nonempty"])
    assert n >= 32
    if "expopac" in options:
        assert 0 < int(np.count_nonzero(cs.d["thick"] == cc.CELL_THICK)) < n
    eng = engine_mod.Engine(model, preset=options)
    eng.set_cellstate(cs, ts)
    assert eng.cache_tiles()[0] == 1
    _compare_cells(eng, oracle, model, cs, ts, options, f"{options} 4^3", range(n))
    eng.close()
    if options == "classic":
        model, cs, ts, aux = synth.build("small", ncoord=6, gridtype=abi.GRID_SPHERICAL1D, options=options)
        assert int(model["npts_nonempty"]) == 6
        eng = engine_mod.Engine(model, preset=options)
        eng.set_cellstate(cs, ts)
        _compare_cells(eng, oracle, model, cs, ts, options, f"{options} 6 shells", range(6))
        eng.close()


def test_the_views_refuse_what_they_cannot_give(engine_mod):
    model, cs, ts, aux = synth.build("small", ncoord=4)
    eng = engine_mod.Engine(model)
    eng.set_cellstate(cs, ts)
    n = int(model["npts_nonempty"])
    for bad in (lambda: eng.debug_cellcache_array(n, "line_dpop"), lambda: eng.debug_cellcache_array(-1, "line_dpop"),
                lambda: eng.debug_cellcache_array(0, "nt_ionratecoeff"), lambda: eng.debug_cellcache_array(0, "expansionopacities")):
        with pytest.raises(engine_mod.EngineError):
            bad()
    import ctypes as C
    buf, written = np.zeros(4), C.c_int64(-1)
    for which, nbytes in ((abi.CC_ARRAYS["line_dpop"][0], 8), (len(abi.CC_ARRAYS), buf.nbytes), (-1, buf.nbytes)):  # a short buffer, two unknown enumerators
        assert eng.L.artis_amd_debug_cellcache_array(eng.h, 0, which, buf.ctypes.data_as(C.c_void_p), nbytes, C.byref(written)) != 0
        assert not buf.any()
    eng.close()
    eng = engine_mod.Engine(model, config=dict(keep_line_dpop=0))  # the factors formed on the fly: no such rows
    eng.set_cellstate(cs, ts)
    with pytest.raises(engine_mod.EngineError):
        eng.debug_cellcache_array(0, "line_dpop")
    assert len(eng.debug_cellcache_array(0, "bf_colion")) == int(model["nphixstargets_total"])
    eng.close()
    model, cs, ts, aux = synth.build("small", ncoord=4, options="kilonova_expopac", host_expopac=True)  # the host's tables: not the engine's to show
    eng = engine_mod.Engine(model, preset="kilonova_expopac")
    eng.set_cellstate(cs, ts)
    with pytest.raises(engine_mod.EngineError):
        eng.debug_cellcache_array(0, "expansionopacities")
    eng.close()


@pytest.mark.parametrize("options", cc.EDGE_BUILDS)
def test_edge_cells_match_oracle(engine_mod, oracle, options):
    """One edge per cell (cellcache_common.apply_edges): thick, an element without mass, one ion carrying its element, T_e at either end of the
    tables, W = 0, nne = 1e-3, T_R far below T_e, T_R = T_e = T_J with W = 1, a photoionisation renormalisation of 0. The oracle alone was
    run on each first (tests/test_cellcache_rules.py asserts it again): it fails on none and every entry it gives is finite, so all ten are
    comparison cases, compared in full like any other cell, and there is no refusal case to list. Two cells behind the edges go with them."""
    model, cs, ts, aux = synth.build("small", ncoord=4, options=options)
    edges = cc.apply_edges(model, cs, options)
    eng = engine_mod.Engine(model, preset=options)
    eng.set_cellstate(cs, ts)
    _compare_cells(eng, oracle, model, cs, ts, options, f"{options} edges {edges}", range(len(cc.EDGES) + 2))
    eng.close()


def _shape_case(engine_mod, oracle, monkeypatch, name, cells):
    monkeypatch.setitem(synth.PRESETS, name, cc.SHAPES[name])
    model, cs, ts, aux = synth.build(name, ncoord=2)
    cc.assert_shape(name, model)
    eng = engine_mod.Engine(model)
    eng.set_cellstate(cs, ts)
    assert eng.cache_tiles()[0] == 1
    n = int(model["npts_nonempty"])
    _compare_cells(eng, oracle, model, cs, ts, "classic", f"{name} 2^3", [c % n for c in cells])
    return eng


def test_more_than_4096_continua(engine_mod, oracle, monkeypatch):
    """Three iron-group elements of five ions with 350 levels each: more than 4096 continua and not a multiple of 64 of them, so k_keptlist
    takes a second trip over the bitmap words (nkeepwords > 64) and k_allcont writes a last word that is partly empty. 2^3 cells, two of
    them against the oracle."""
    eng = _shape_case(engine_mod, oracle, monkeypatch, "manycont", (0, -1))
    assert len(eng.debug_cellcache_array(0, "allcont_keepprefix")) > 64
    eng.close()


def test_fewer_continua_than_a_wave(engine_mod, oracle, monkeypatch):
    _shape_case(engine_mod, oracle, monkeypatch, "one_ion", range(8)).close()


def test_directions_longer_than_a_block(engine_mod, oracle, monkeypatch):
    """one ion pair with 420 levels: directions of more than 256 transitions, whose rates k_matrans sums 64 terms at a time and whose filters
    k_mafilter_long writes (test_filter_records_of_long_directions_... holds three arrays of such a model to the oracle; here the whole row)"""
    _shape_case(engine_mod, oracle, monkeypatch, "longdir", (4,)).close()


def test_more_items_than_a_16_lane_group(engine_mod, oracle, monkeypatch):
    """k_macroatom_recomb sums a level's recombination list and the cooling chain an ion's upward transitions in rows of 16 lanes, 16 items
    at a time with the sum carried from one 16 to the next. `small` has recombination lists of at most 12 pairs; here every list has more
    than 16, every ion more than 16 levels with upward transitions, and there are more than 16 ions (cellcache_common.assert_shape)."""
    _shape_case(engine_mod, oracle, monkeypatch, "wide", (0, -1)).close()


def test_fill_in_batches(engine_mod, oracle):
    """the population's scratch holds 11 cells' cooling terms: the 32 cells are filled in three batches; the last cell of a batch and the
    first of the next, at both seams, and the last cell"""
    model, cs, ts, aux = synth.build("small", ncoord=4)
    n, per = int(model["npts_nonempty"]), 8 * int(model["nlines"])
    config = dict(pop_scratch_bytes=11 * per + 8)
    batch = (engine_mod.plan(model, config=config, free_bytes=1 << 36)["pop_scratch_bytes"] - 64) // per
    assert batch == 11 and -(-n // batch) >= 3
    eng = engine_mod.Engine(model, config=config)
    eng.set_cellstate(cs, ts)
    assert eng.cache_tiles()[0] == 1
    _compare_cells(eng, oracle, model, cs, ts, "classic", "small 4^3 in batches of 11", (batch - 1, batch, 2 * batch - 1, 2 * batch, n - 1))
    eng.close()


@pytest.mark.parametrize("options", ["classic", "classic_expopac_therm"])
def test_tiled_rows_equal_untiled_rows(engine_mod, oracle, options):
    """A cache of two tiles fills the cells it is asked for (a fill of listed cells, through the row table), in the order asked: the last cell
    gets row 0, so no row here is its cell's index. Every array of those rows equals the one-tile engine's rows of the same cells byte for
    byte -- and so meets the oracle as they do (the cells are among those of the first test)."""
    model, cs, ts, aux = synth.build("small", ncoord=4, thick_below_v=cc.THICK_BELOW_V if "expopac" in options else 0.0, options=options)
    n = int(model["npts_nonempty"])
    one = engine_mod.Engine(model, preset=options)
    one.set_cellstate(cs, ts)
    tiles = one.cache_tiles()
    assert tiles[0] == 1
    two = engine_mod.Engine(model, preset=options, config=dict(cache_budget_bytes=int(tiles[2]) * (n // 2 + 1) + 4096, ma_hot_fraction=1.0,
                                                               ma_pool_fraction=1.0))
    two.set_cellstate(cs, ts)
    assert two.cache_tiles()[0] == 2 and two.cache_tiles()[1] < n - 1
    cells = [n - 1, 5, 0, n // 2, 6]  # (cell n - 1 first: its row is 0; cell 0 third: its row is 2)
    rows = {c: cc.view_row(two, c, options) for c in cells}  # ... each made resident after the ones before it
    rows_again = {c: cc.view_row(two, c, options) for c in cells}  # (now resident: no fill)
    for c in cells:
        want = cc.view_row(one, c, options)
        assert set(want) == set(rows[c]) == set(rows_again[c])
        for name, a in want.items():
            if name in ("allcont_keptlist", "allcont_keptpair"):  # (places behind the kept continua are never written: not part of the row's content)
                k = int(np.unpackbits(want["allcont_keepbits_row"].view(np.uint8)).sum())
                a, b, b2 = a[:k], rows[c][name][:k], rows_again[c][name][:k]
            else:
                b, b2 = rows[c][name], rows_again[c][name]
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes() == np.asarray(b2).tobytes(), f"{options} cell {c}: {name}"
    _compare_cells(two, oracle, model, cs, ts, options, f"{options} two tiles", (n - 1, 0))
    one.close()
    two.close()
