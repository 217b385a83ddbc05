"""The cell cache's population on the host (tests/hostemu: the bodies of physics.h in the kernels' launch order) against the oracle, bit for
bit: every array of a row (cellcache_common.py), in every build whose options change a body of the population, in every non-empty cell, and
in the cells whose state is an edge. What the host emulation cannot vouch for -- the wave-cooperative kernels themselves -- is
tests/test_gpu_cellcache.py's, which shares the cases and the comparison."""
import numpy as np
import pytest

import cellcache_common as cc
import hostemu_binding as emu
from artis_amd import abi, synth


def _compare_all_cells(oracle, model, cs, ts, options, what, cells=None):
    view = emu.CellCacheView(model, cs, ts, preset=options)
    assert view.error == 0, f"{what}: the emulated population raised error flag {view.error}"
    for c in (range(int(model["npts_nonempty"])) if cells is None else cells):
        row = cc.view_row(view, c, options)
        ref = cc.oracle_row(oracle, model, cs, ts, c, options)
        cc.check_against_oracle(row, ref, model, cs, c, options, True, f"{what} cell {c}")
        cc.check_derived(row, model, emu.cool_guide_row, f"{what} cell {c}")
    view.close()


@pytest.mark.parametrize("options", cc.BUILDS)
def test_every_array_of_every_cell_bit_exact(oracle, options):
    """`small` on 4^3 cells (the innermost thick in the expansion builds, so that they meet cells without tables) and, for one build, on 6 shells"""
    model, cs, ts, aux = synth.build("small", ncoord=4, thick_below_v=cc.THICK_BELOW_V if "expopac" in options else 0.0, options=options)
    assert int(model["npts_nonempty"]) >= 32
    if "expopac" in options:
        assert 0 < int(np.count_nonzero(cs.d["thick"] == cc.CELL_THICK)) < int(model["npts_nonempty"])
    _compare_all_cells(oracle, model, cs, ts, options, f"{options} 4^3")
    if options == "classic":
        model, cs, ts, aux = synth.build("small", ncoord=6, gridtype=abi.GRID_SPHERICAL1D, options=options)
        assert int(model["npts_nonempty"]) == 6
        _compare_all_cells(oracle, model, cs, ts, options, f"{options} 6 shells")


@pytest.mark.parametrize("name", sorted(cc.SHAPES))
def test_shapes_of_the_untaken_loop_trips_bit_exact(oracle, monkeypatch, name):
    """the atomic data the GPU tests use for the loop trips `small` never takes: the sequential bodies take no such trips, but the arrays
    they leave are what the kernels have to reproduce there, and the shapes' properties are asserted here as well"""
    monkeypatch.setitem(synth.PRESETS, name, cc.SHAPES[name])
    model, cs, ts, aux = synth.build(name, ncoord=2)
    cc.assert_shape(name, model)
    _compare_all_cells(oracle, model, cs, ts, "classic", f"{name} 2^3", cells=(0, int(model["npts_nonempty"]) - 1))


@pytest.mark.parametrize("options", cc.EDGE_BUILDS)
def test_edge_cells_bit_exact(oracle, options):
    """One edge per cell (cellcache_common.apply_edges). The oracle alone was run on each first: it fails on none of them and every entry it
    gives is finite, so every edge is a comparison case and none a refusal case (asserted here, so that a change of the synthetic state that
    turns one into a refusal is seen). The cells behind the edges are compared too: the helper must leave them alone."""
    model, cs, ts, aux = synth.build("small", ncoord=4, options=options)
    untouched = {k: np.array(v, copy=True) for k, v in cs.d.items() if isinstance(v, np.ndarray)}
    edges = cc.apply_edges(model, cs, options)
    n = len(cc.EDGES)
    for k, v in untouched.items():
        per = v.size // int(model["npts_nonempty"])
        if per * int(model["npts_nonempty"]) == v.size and per > 0:
            assert np.array_equal(v.reshape(int(model["npts_nonempty"]), per)[n:], cs.d[k].reshape(int(model["npts_nonempty"]), per)[n:]), k
    for name, c in edges.items():
        ref = cc.oracle_row(oracle, model, cs, ts, c, options)  # (raises where the oracle fails)
        for k, v in ref.items():
            assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), f"{options} edge {name}: the oracle's {k} is not finite"
    _compare_all_cells(oracle, model, cs, ts, options, f"{options} edges", cells=range(n + 2))
