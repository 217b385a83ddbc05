// residency_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The two operations of artis_amd/csrc/cache_residency.h -- rows for a wanted set of cells, and the choice of the cells a visit of a tiled cache
// makes resident -- behind a flat C interface. tests/test_cache_residency_rules.py holds them to a numpy restatement of the rules.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../artis_amd/csrc/cache_residency.h"

using namespace artis_residency;

extern "C" {

// a row table of `nrows` rows for `ncell` non-empty cells, no cell resident
void *res_host_new(int64_t ncell, int64_t nrows) {
  Residency *r = new Residency;
  r->tile_cells = nrows;
  r->init(ncell);
  return r;
}
void res_host_free(void *h) { delete (Residency *)h; }
void res_host_reset(void *h) { ((Residency *)h)->reset(); }
// krow[ncell], rowcell[nrows]: the tables as they stand
void res_host_tables(void *h, int32_t *krow, int32_t *rowcell) {
  const Residency &r = *(const Residency *)h;
  std::memcpy(krow, r.krow.data(), sizeof(int32_t) * r.krow.size());
  std::memcpy(rowcell, r.rowcell.data(), sizeof(int32_t) * r.rowcell.size());
}
// Residency::assign: returns its code (0: done); fresh[nwant] receives the *nfresh cells that got a row
int res_host_assign(void *h, const int32_t *want, int64_t nwant, int32_t *fresh, int64_t *nfresh) {
  std::vector<int32_t> f;
  const int rc = ((Residency *)h)->assign(std::vector<int32_t>(want, want + nwant), f);
  *nfresh = (int64_t)f.size();
  if (!f.empty()) std::memcpy(fresh, f.data(), sizeof(int32_t) * f.size());
  return rc;
}
void res_host_give_back(void *h, const int32_t *fresh, int64_t nfresh) { ((Residency *)h)->give_back(std::vector<int32_t>(fresh, fresh + nfresh)); }
// choose_cells on a grid of ncoordgrid[0] x [1] x [2] cells (strides as model_build.h makes them: the first axis runs fastest) whose non-empty cells
// propcell_nonemptymgi numbers; waiting[ncell]. Returns the number of chosen cells, written to want[ncell].
int64_t res_host_choose(void *h, const int32_t *waiting, int64_t ncell, int64_t tile_block, int sparse_fill, int64_t sparse_max_listed, int64_t win_lo,
                        int ndim, const int32_t *ncoordgrid, const int32_t *propcell_nonemptymgi, int32_t *want, int64_t *holds, int *sparse) {
  const int32_t stride[3] = {1, ncoordgrid[0], ncoordgrid[0] * ncoordgrid[1]};
  const int ngrid = ncoordgrid[0] * ncoordgrid[1] * ncoordgrid[2];
  std::vector<int32_t> cell_grid((size_t)ncell, 0);
  for (int g = 0; g < ngrid; g++)
    if (propcell_nonemptymgi[g] >= 0) cell_grid[(size_t)propcell_nonemptymgi[g]] = g;
  const GridView grid{ndim, ncoordgrid, stride, propcell_nonemptymgi, cell_grid.data()};
  std::vector<int32_t> w;
  bool sp = false;
  choose_cells(*(Residency *)h, std::vector<int32_t>(waiting, waiting + ncell), ncell, tile_block, sparse_fill != 0, sparse_max_listed, win_lo, grid, w,
               holds, &sp);
  *sparse = sp ? 1 : 0;
  if (!w.empty()) std::memcpy(want, w.data(), sizeof(int32_t) * w.size());
  return (int64_t)w.size();
}

}  // extern "C"
