// cache_residency.h -- which cells of a tiled cell cache hold rows: plain host C++17 over a few integer vectors, no HIP, nothing of the engine.
// stage_cellcache.h makes the copies and the fills these decisions ask for; tests/residency_host compiles this file for x86.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace artis_residency {

// The row table of a tiled cache: which cell's cache each row holds, populated for the current cell state (physics.h Env::krow_tab).
struct Residency {
  int64_t tile_cells = 0;        // rows: the non-empty cells that are resident at a time
  std::vector<int32_t> krow;     // [npts_nonempty] row of the cell, -1: not resident
  std::vector<int32_t> rowcell;  // [tile_cells] cell of the row, -1: free
  std::vector<int32_t> wanted;   // [npts_nonempty] stamp of the last assign() that asked for the cell (> 0), or of the last sparse choice that listed it (< 0)
  int32_t want_stamp = 0;

  enum { OK = 0, MORE_CELLS_THAN_ROWS, NO_ROW_LEFT };

  // the tables of `ncell` non-empty cells, no cell resident
  void init(int64_t ncell) {
    krow.assign((size_t)ncell, -1);
    wanted.assign((size_t)ncell, 0);
    rowcell.assign((size_t)tile_cells, -1);
  }
  // no cell is resident (a new cell state: what the rows hold belongs to the old one)
  void reset() {
    std::fill(krow.begin(), krow.end(), -1);
    std::fill(rowcell.begin(), rowcell.end(), -1);
  }
  // Rows for the cells want[0..) (at most tile_cells of them). A wanted cell that is resident keeps its row; the others take the free rows, then the
  // rows of cells that are not wanted (which stay resident as long as nobody needs their rows), in row order. fresh: the cells that got a row, in
  // the order of want -- they are to be filled.
  int assign(const std::vector<int32_t> &want, std::vector<int32_t> &fresh) {
    fresh.clear();
    if ((int64_t)want.size() > tile_cells) return MORE_CELLS_THAN_ROWS;
    const int32_t stamp = ++want_stamp;
    for (const int32_t c : want) {
      wanted[(size_t)c] = stamp;
      if (krow[(size_t)c] < 0) fresh.push_back(c);
    }
    size_t k = 0;
    for (int pass = 0; pass < 2 && k < fresh.size(); pass++)
      for (size_t r = 0; r < rowcell.size() && k < fresh.size(); r++) {
        const int32_t held = rowcell[r];
        if (pass == 0 ? held >= 0 : (held < 0 || wanted[(size_t)held] == stamp)) continue;
        if (held >= 0) krow[(size_t)held] = -1;
        rowcell[r] = fresh[k];
        krow[(size_t)fresh[k]] = (int32_t)r;
        k++;
      }
    return k < fresh.size() ? NO_ROW_LEFT : OK;
  }
  // the fill of `fresh` failed: what the rows of the new cells hold is not to be used
  void give_back(const std::vector<int32_t> &fresh) {
    for (const int32_t c : fresh) {
      rowcell[(size_t)krow[(size_t)c]] = -1;
      krow[(size_t)c] = -1;
    }
  }
};

// what choose_cells() needs of the grid
struct GridView {
  int ndim;                                 // 1 (spherical shells), 2 (cylindrical) or 3
  const int32_t *ncoordgrid, *coordstride;  // [3] cells per axis; grid-index step per axis
  const int32_t *propcell_nonemptymgi;      // [ngrid] the non-empty cell of a grid cell, -1: empty
  const int32_t *cell_grid;                 // [npts_nonempty] the grid cell of a non-empty cell (the inverse)
};

// Which cells should be resident for the next visit of a tiled run? waiting[c]: packets that wait in non-empty cell c (k_count_waiting), c < ncell_all.
//  - few packets wait (at most sparse_max_listed of them, in less than half as many cells as there are rows): the cells in which they wait and the cells
//    around those, one step in every grid direction (an r-packet crosses a few cells per visit) -- a "sparse" visit
//  - win_lo >= 0: the window of tile_cells consecutive cells that begins there
//  - tile_block == 0: the window of tile_cells consecutive cells in which most packets wait
//  - else: the blocks of tile_block consecutive cells in which most packets wait, wherever they lie, as many as there are rows for
// *holds: the packets that wait in the chosen cells.
inline void choose_cells(Residency &res, const std::vector<int32_t> &waiting, int64_t ncell_all, int64_t tile_block, bool sparse_fill,
                         int64_t sparse_max_listed, int64_t win_lo, const GridView &grid, std::vector<int32_t> &want, int64_t *holds, bool *sparse) {
  const int64_t nrows = res.tile_cells;
  want.clear();
  *sparse = false;
  *holds = 0;
  int64_t lo = win_lo;
  if (win_lo < 0 && tile_block > 0 && tile_block < nrows) {
    const int64_t B = tile_block, nblk = (ncell_all + B - 1) / B;
    std::vector<std::pair<int64_t, int64_t>> score((size_t)nblk);
    for (int64_t b = 0; b < nblk; b++) {
      int64_t sum = 0;
      for (int64_t c = b * B; c < std::min(ncell_all, (b + 1) * B); c++) sum += waiting[(size_t)c];
      score[(size_t)b] = {-sum, b};
    }
    std::sort(score.begin(), score.end());
    for (const auto &sb : score) {
      const int64_t c0 = sb.second * B, c1 = std::min(ncell_all, c0 + B);
      if (sb.first == 0 || (int64_t)want.size() + (c1 - c0) > nrows) break;
      for (int64_t c = c0; c < c1; c++) want.push_back((int32_t)c);
      *holds -= sb.first;
    }
    std::sort(want.begin(), want.end());
  } else {
    if (win_lo < 0) {
      int64_t sum = 0, best = -1;
      lo = 0;
      for (int64_t c = 0; c < ncell_all; c++) {
        sum += waiting[(size_t)c];
        if (c >= nrows) sum -= waiting[(size_t)(c - nrows)];
        if ((c >= nrows - 1 || c == ncell_all - 1) && sum > best) {
          best = sum;
          lo = std::max<int64_t>(0, c - nrows + 1);
        }
      }
      lo = std::min<int64_t>(lo, std::max<int64_t>(0, ncell_all - nrows));
    }
    for (int64_t c = lo; c < std::min(ncell_all, lo + nrows); c++) {
      want.push_back((int32_t)c);
      *holds += waiting[(size_t)c];
    }
  }
  if (!sparse_fill || *holds > sparse_max_listed) return;
  // a sparse visit: of the chosen cells, those in which packets wait, and the cells around them (whichever cells those are)
  std::vector<int32_t> few;
  const int32_t stamp = -(++res.want_stamp);  // (marks of this choice: negative, never those of assign())
  std::vector<int32_t> &mark = res.wanted;
  for (const int32_t c : want) {
    if (waiting[(size_t)c] <= 0) continue;
    const int g = grid.cell_grid[(size_t)c];
    int lo3[3] = {0, 0, 0}, hi3[3] = {0, 0, 0};
    for (int d = 0; d < grid.ndim; d++) {
      const int idx = (g / grid.coordstride[d]) % grid.ncoordgrid[d];
      lo3[d] = idx > 0 ? -1 : 0;
      hi3[d] = idx < grid.ncoordgrid[d] - 1 ? 1 : 0;
    }
    for (int dz = lo3[2]; dz <= hi3[2]; dz++)
      for (int dy = lo3[1]; dy <= hi3[1]; dy++)
        for (int dx = lo3[0]; dx <= hi3[0]; dx++) {
          const int cn = grid.propcell_nonemptymgi[g + (dx * grid.coordstride[0]) + (dy * grid.coordstride[1]) + (dz * grid.coordstride[2])];
          if (cn < 0 || mark[(size_t)cn] == stamp) continue;
          mark[(size_t)cn] = stamp;
          few.push_back(cn);
        }
  }
  if (few.empty() || (int64_t)few.size() * 2 >= nrows) return;
  want.swap(few);
  *sparse = true;
}

}  // namespace artis_residency
