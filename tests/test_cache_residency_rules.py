"""The residency rules of a tiled cell cache (artis_amd/csrc/cache_residency.h) compiled for x86 (tests/residency_host), against a numpy
restatement of the rules as the comments above choose_cells() and make_resident() state them:

 - rows: a wanted cell that is resident keeps its row; the others take the free rows, then the rows of cells that are not wanted, in row order;
 - window: the first window of `rows` consecutive cells with the strictly largest number of waiting packets, no further up than the last full window;
 - blocks: blocks of `tile_block` consecutive cells by waiting packets, then block index, taken until one has no packet or does not fit;
 - sparse: the chosen cells in which packets wait and the existing cells around them, one step per axis, diagonals included -- taken only when the
   visit holds at most `sparse_max_listed` packets and the cells are fewer than half the rows.
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import host_build

HERE = os.path.dirname(os.path.abspath(__file__))
_HOSTDIR = os.path.join(HERE, "residency_host")
_LIB = []
I32P = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


def _lib():
    if not _LIB:
        L = host_build.load(_HOSTDIR, lambda p: "libresidency_host.so", "classic")
        L.res_host_new.restype = C.c_void_p
        L.res_host_new.argtypes = [C.c_int64, C.c_int64]
        L.res_host_free.argtypes = [C.c_void_p]
        L.res_host_reset.argtypes = [C.c_void_p]
        L.res_host_tables.argtypes = [C.c_void_p, I32P, I32P]
        L.res_host_assign.argtypes = [C.c_void_p, I32P, C.c_int64, I32P, C.POINTER(C.c_int64)]
        L.res_host_give_back.argtypes = [C.c_void_p, I32P, C.c_int64]
        L.res_host_choose.restype = C.c_int64
        L.res_host_choose.argtypes = [C.c_void_p, I32P, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, I32P, I32P, I32P,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int)]
        _LIB.append(L)
    return _LIB[0]


class Grid:
    """dims[0] x dims[1] x dims[2] grid cells, the first axis fastest; the cells of `empty` hold nothing"""

    def __init__(self, ndim, dims, empty):
        self.ndim, self.dims = ndim, tuple(dims)
        ngrid = int(np.prod(dims))
        self.nonemptymgi = np.full(ngrid, -1, np.int32)
        full = [g for g in range(ngrid) if g not in set(empty)]
        self.nonemptymgi[full] = np.arange(len(full), dtype=np.int32)
        self.cell_grid = np.array(full)
        self.ncell = len(full)

    def around(self, c):
        """the non-empty cells at most one step away from cell c along every axis (c itself among them)"""
        pos = np.unravel_index(self.cell_grid[c], self.dims, order="F")
        out = set()
        for step in itertools.product((-1, 0, 1), repeat=self.ndim):
            p = [pos[d] + (step[d] if d < self.ndim else 0) for d in range(3)]
            if all(0 <= p[d] < self.dims[d] for d in range(3)):
                n = self.nonemptymgi[np.ravel_multi_index(p, self.dims, order="F")]
                if n >= 0:
                    out.add(int(n))
        return out


GRIDS = {
    "1d": Grid(1, (9, 1, 1), empty=(3, 8)),
    "2d": Grid(2, (4, 5, 1), empty=(0, 6, 19)),
    "3d": Grid(3, (4, 4, 4), empty=(0, 3, 21, 22, 42, 63)),
}
LINE9 = Grid(1, (10, 1, 1), empty=(4,))  # nine cells in a row for the window and block cases (their choice does not look at the grid)


class Table:
    """a row table of the harness"""

    def __init__(self, ncell, nrows):
        self.ncell, self.nrows = ncell, nrows
        self.h = _lib().res_host_new(ncell, nrows)

    def close(self):
        _lib().res_host_free(self.h)

    def tables(self):
        krow, rowcell = np.zeros(self.ncell, np.int32), np.zeros(self.nrows, np.int32)
        _lib().res_host_tables(self.h, krow, rowcell)
        return krow, rowcell

    def assign(self, want):
        want = np.ascontiguousarray(want, np.int32)
        fresh, n = np.zeros(max(1, len(want)), np.int32), C.c_int64(0)
        rc = _lib().res_host_assign(self.h, want, len(want), fresh, C.byref(n))
        return rc, [int(c) for c in fresh[: n.value]]

    def reset(self):
        _lib().res_host_reset(self.h)

    def give_back(self, fresh):
        _lib().res_host_give_back(self.h, np.ascontiguousarray(fresh, np.int32), len(fresh))

    def choose(self, grid, waiting, tile_block=0, sparse_fill=True, sparse_max=16384, win_lo=-1):
        waiting = np.ascontiguousarray(waiting, np.int32)
        assert len(waiting) == grid.ncell == self.ncell
        want, holds, sparse = np.zeros(self.ncell, np.int32), C.c_int64(0), C.c_int(0)
        n = _lib().res_host_choose(self.h, waiting, self.ncell, tile_block, int(sparse_fill), sparse_max, win_lo, grid.ndim,
                                   np.array(grid.dims, np.int32), grid.nonemptymgi, want, C.byref(holds), C.byref(sparse))
        return [int(c) for c in want[:n]], holds.value, bool(sparse.value)


@pytest.fixture
def table():
    made = []

    def make(ncell, nrows):
        made.append(Table(ncell, nrows))
        return made[-1]

    yield make
    for t in made:
        t.close()


def ref_choose(grid, waiting, nrows, tile_block=0, sparse_fill=True, sparse_max=16384, win_lo=-1):
    """the rules restated: (cells, packets they hold, sparse?); the cells of a sparse choice as a set"""
    waiting = np.asarray(waiting, np.int64)
    ncell = len(waiting)
    if win_lo < 0 and 0 < tile_block < nrows:
        B = tile_block
        sums = [int(waiting[b * B:(b + 1) * B].sum()) for b in range(-(-ncell // B))]
        want, holds = [], 0
        for b in sorted(range(len(sums)), key=lambda b: (-sums[b], b)):
            cells = list(range(b * B, min(ncell, (b + 1) * B)))
            if sums[b] == 0 or len(want) + len(cells) > nrows:
                break
            want += cells
            holds += sums[b]
        want.sort()
    else:
        lo = win_lo
        if win_lo < 0:
            full = [int(waiting[l:l + nrows].sum()) for l in range(max(1, ncell - nrows + 1))]
            lo = int(np.argmax(full))  # (the first of equal maxima)
        want = list(range(lo, min(ncell, lo + nrows)))
        holds = int(waiting[want].sum())
    if not sparse_fill or holds > sparse_max:
        return want, holds, False
    few = set()
    for c in want:
        if waiting[c] > 0:
            few |= grid.around(c)
    if not few or 2 * len(few) >= nrows:
        return want, holds, False
    return few, holds, True


def check_choice(t, grid, waiting, **kw):
    want, holds, sparse = t.choose(grid, waiting, **kw)
    rwant, rholds, rsparse = ref_choose(grid, waiting, t.nrows, **kw)
    assert (holds, sparse) == (rholds, rsparse)
    if sparse:
        assert len(set(want)) == len(want) and set(want) == rwant
    else:
        assert want == rwant
    return want, holds, sparse


# ---- window choice: rows = 3 of 9 cells
@pytest.mark.parametrize("waiting, win_lo, cells, holds", [
    ([0, 1, 0, 2, 5, 4, 0, 1, 0], -1, [3, 4, 5], 11),   # a unique maximum
    ([0, 4, 3, 0, 0, 3, 4, 0, 0], -1, [0, 1, 2], 7),    # windows 0, 1, 4 and 5 tie: the lowest
    ([0, 0, 0, 0, 0, 0, 0, 0, 9], -1, [6, 7, 8], 9),    # the maximum in the last stretch: the last full window
    ([0, 0, 0, 0, 0, 0, 0, 2, 9], -1, [6, 7, 8], 11),
    ([0, 0, 0, 0, 0, 0, 0, 0, 0], -1, [0, 1, 2], 0),    # nothing waits
    ([9, 9, 9, 0, 1, 0, 0, 0, 0], 3, [3, 4, 5], 1),     # a fixed window
    ([9, 9, 9, 0, 1, 0, 0, 0, 2], 6, [6, 7, 8], 2),
])
def test_window_choice(table, waiting, win_lo, cells, holds):
    t = table(9, 3)
    got = check_choice(t, LINE9, waiting, sparse_fill=False, win_lo=win_lo)
    assert got == (cells, holds, False)


# ---- block choice: blocks of 2 cells, 5 rows: {0,1} {2,3} {4,5} {6,7} {8}
@pytest.mark.parametrize("waiting, cells, holds", [
    ([1, 0, 0, 7, 2, 2, 3, 3, 1], [2, 3, 6, 7], 13),   # blocks 1 and 3 fit; block 2 is refused for lack of room, and the choice ends there
    ([1, 0, 0, 7, 3, 2, 3, 3, 4], [2, 3, 6, 7], 13),   # ... also where a later, smaller block would still fit
    ([0, 0, 0, 7, 0, 0, 3, 3, 6], [2, 3, 6, 7, 8], 19),  # the short last block as the third
    ([3, 0, 0, 0, 3, 0, 0, 0, 0], [0, 1, 4, 5], 6),    # equal blocks: by index; a block without packets ends the choice
    ([0, 0, 0, 0, 0, 0, 0, 2, 0], [6, 7], 2),
    ([0, 0, 0, 0, 0, 0, 0, 0, 0], [], 0),
])
def test_block_choice(table, waiting, cells, holds):
    t = table(9, 5)
    got = check_choice(t, LINE9, waiting, tile_block=2, sparse_fill=False)
    assert got == (cells, holds, False)
    assert got[0] == sorted(got[0]) and got[1] == sum(waiting[c] for c in got[0])


def test_block_as_large_as_the_rows_is_a_window(table):
    t = table(9, 3)
    assert check_choice(t, LINE9, [0, 1, 0, 2, 5, 4, 0, 1, 0], tile_block=3, sparse_fill=False)[0] == [3, 4, 5]


# ---- sparse choice
@pytest.mark.parametrize("name", list(GRIDS))
def test_sparse_choice_is_the_waiting_cells_and_the_cells_around_them(table, name):
    grid = GRIDS[name]
    assert (grid.nonemptymgi < 0).any()
    sizes = set()
    for c in range(grid.ncell):
        size = len(grid.around(c))
        sizes.add(size)
        waiting = np.zeros(grid.ncell, np.int32)
        waiting[c] = 5
        # rejected at 2 x size >= rows, taken with one row more
        for nrows, taken in ((2 * size, False), (2 * size + 1, True)):
            t = table(grid.ncell, nrows)
            want, holds, sparse = check_choice(t, grid, waiting)
            assert sparse == taken and holds == 5 and c in want
            assert set(want) == grid.around(c) if taken else len(want) == min(nrows, grid.ncell)
    assert len(sizes) > 1  # (cells at the edge or beside empty cells have fewer neighbours)
    # several waiting cells, some of them neighbours of each other: no cell twice
    rng = np.random.default_rng(5)
    for _ in range(20):
        waiting = np.zeros(grid.ncell, np.int32)
        waiting[rng.choice(grid.ncell, size=3, replace=False)] = rng.integers(1, 9, size=3)
        for nrows in (grid.ncell - 1, grid.ncell // 2, 4):
            check_choice(table(grid.ncell, nrows), grid, waiting)


def test_sparse_choice_limits(table):
    grid = GRIDS["2d"]
    c = int(grid.nonemptymgi[np.ravel_multi_index((3, 0, 0), grid.dims, order="F")])
    waiting = np.zeros(grid.ncell, np.int32)
    waiting[c] = 5
    nrows = grid.ncell - 1
    window = ref_choose(grid, waiting, nrows, sparse_fill=False)[0]
    assert len(window) == nrows and 2 * len(grid.around(c)) < nrows
    assert check_choice(table(grid.ncell, nrows), grid, waiting, sparse_max=5)[2]           # holds == sparse_max_listed: sparse
    assert check_choice(table(grid.ncell, nrows), grid, waiting, sparse_max=4) == (window, 5, False)  # more: the window
    assert check_choice(table(grid.ncell, nrows), grid, waiting, sparse_fill=False) == (window, 5, False)
    assert check_choice(table(grid.ncell, nrows), grid, np.zeros(grid.ncell, np.int32)) == (window, 0, False)  # nothing waits: the window
    # only the waiting cells of the chosen window count: a fixed window elsewhere ignores the cell
    t = table(grid.ncell, 4)
    lo = 0 if c >= 4 else grid.ncell - 4
    assert check_choice(t, grid, waiting, win_lo=lo) == (list(range(lo, lo + 4)), 0, False)


@pytest.mark.parametrize("name", list(GRIDS))
def test_choices_and_assignments_share_one_mark_vector(table, name):
    """the marks of a sparse choice and the stamps of an assignment live in one vector: neither is mistaken for the other, however they alternate"""
    grid = GRIDS[name]
    nrows = grid.ncell - 1
    t = table(grid.ncell, nrows)
    a, b = np.zeros(grid.ncell, np.int32), np.zeros(grid.ncell, np.int32)
    a[0], b[2] = 3, 4  # their surroundings overlap
    assert grid.around(0) & grid.around(2)
    model = RowModel(grid.ncell, nrows)
    for waiting in (a, a, b, a, b, b, a):
        want, _, sparse = check_choice(t, grid, waiting)
        assert sparse
        rc, fresh = t.assign(want)
        assert rc == 0 and fresh == model.assign(want)
        model.check(t)
        check_choice(t, grid, waiting)  # (a choice between two assignments)


# ---- row assignment
class RowModel:
    def __init__(self, ncell, nrows):
        self.krow, self.rowcell = np.full(ncell, -1), np.full(nrows, -1)

    def assign(self, want):
        fresh = [c for c in want if self.krow[c] < 0]
        rows = [r for r in range(len(self.rowcell)) if self.rowcell[r] < 0]
        rows += [r for r in range(len(self.rowcell)) if self.rowcell[r] >= 0 and self.rowcell[r] not in want]
        for c, r in zip(fresh, rows):
            if self.rowcell[r] >= 0:
                self.krow[self.rowcell[r]] = -1
            self.rowcell[r], self.krow[c] = c, r
        return fresh

    def check(self, t):
        krow, rowcell = t.tables()
        assert (krow == self.krow).all() and (rowcell == self.rowcell).all()


def check_inverse(krow, rowcell):
    for c, r in enumerate(krow):
        assert r < 0 or rowcell[r] == c
    for r, c in enumerate(rowcell):
        assert c < 0 or krow[c] == r


def test_row_assignment(table):
    t = table(9, 4)
    model = RowModel(9, 4)
    for want in ([0, 1, 2], [2, 3], [5, 4, 2], [5, 6, 7, 8], [0]):
        krow0, rowcell0 = t.tables()
        rc, fresh = t.assign(want)
        krow, rowcell = t.tables()
        assert rc == 0
        check_inverse(krow, rowcell)
        assert all(krow[c] >= 0 for c in want)                                   # every wanted cell is resident,
        assert all(krow[c] == krow0[c] for c in want if krow0[c] >= 0)           # in the row it had, if it had one
        assert fresh == [c for c in want if krow0[c] < 0]                        # the others are reported, in the order of the wanted list
        evicted = [c for c in range(9) if krow0[c] >= 0 and krow[c] < 0]
        assert not set(evicted) & set(want)
        assert not evicted or (rowcell >= 0).all()                               # no cell gives up its row while a row is free
        assert len(evicted) == max(0, len(fresh) - int((rowcell0 < 0).sum()))
        assert fresh == model.assign(want)
        model.check(t)                                                           # free rows first, then unwanted cells' rows in row order
    assert list(t.tables()[1]) == [0, 6, 7, 8]


def test_row_assignment_errors_and_reset(table):
    t = table(9, 4)
    assert t.assign([0, 1, 2]) == (0, [0, 1, 2])
    before = t.tables()
    rc, fresh = t.assign([4, 5, 6, 7, 8])  # more cells than rows
    assert rc != 0 and fresh == []
    assert all((x == y).all() for x, y in zip(before, t.tables()))
    assert t.assign([2, 4, 5]) == (0, [4, 5])
    assert list(t.tables()[1]) == [5, 1, 2, 4]
    t.reset()
    assert (t.tables()[0] == -1).all() and (t.tables()[1] == -1).all()
    assert t.assign([0, 1, 2, 3]) == (0, [0, 1, 2, 3])
    assert t.assign([4, 5, 2]) == (0, [4, 5])
    assert list(t.tables()[1]) == [4, 5, 2, 3]
    # a failed fill: its cells are not resident and their rows are free; the cells they displaced stay out
    t.give_back([4, 5])
    krow, rowcell = t.tables()
    assert list(rowcell) == [-1, -1, 2, 3] and list(krow) == [-1, -1, 2, 3, -1, -1, -1, -1, -1]
    check_inverse(krow, rowcell)
    assert t.assign([7]) == (0, [7]) and list(t.tables()[1]) == [7, -1, 2, 3]
