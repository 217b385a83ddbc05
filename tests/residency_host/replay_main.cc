// replay_main.cc -- TEST HARNESS ONLY. The call sequences of tests/test_cache_residency_rules.py through the flat interface of residency_host.cc, as a
// program of its own to run under the address and undefined-behaviour sanitizers (make replay_sanitized); the test holds the answers to the rules, this
// program only repeats the calls and checks what the cases state outright.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" {
void *res_host_new(int64_t ncell, int64_t nrows);
void res_host_free(void *h);
void res_host_reset(void *h);
void res_host_tables(void *h, int32_t *krow, int32_t *rowcell);
int res_host_assign(void *h, const int32_t *want, int64_t nwant, int32_t *fresh, int64_t *nfresh);
void res_host_give_back(void *h, const int32_t *fresh, int64_t nfresh);
int64_t res_host_choose(void *h, const int32_t *waiting, int64_t ncell, int64_t tile_block, int sparse_fill, int64_t sparse_max_listed, int64_t win_lo,
                        int ndim, const int32_t *ncoordgrid, const int32_t *propcell_nonemptymgi, int32_t *want, int64_t *holds, int *sparse);
}

namespace {
using Cells = std::vector<int32_t>;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      exit(1);                                                       \
    }                                                                \
  } while (0)

struct Grid {
  int ndim;
  int32_t dims[3];
  Cells nonemptymgi;
  int ncell = 0;
  Grid(int ndim_, int nx, int ny, int nz, const Cells &empty) : ndim(ndim_), dims{nx, ny, nz}, nonemptymgi((size_t)(nx * ny * nz), 0) {
    for (const int32_t g : empty) nonemptymgi[(size_t)g] = -1;
    for (int32_t &n : nonemptymgi) n = n < 0 ? -1 : ncell++;
  }
};
struct Choice {
  Cells want;
  int64_t holds;
  bool sparse;
};
Choice choose(void *h, const Grid &g, const Cells &waiting, int64_t tile_block = 0, bool sparse_fill = true, int64_t sparse_max = 16384,
              int64_t win_lo = -1) {
  Choice c{Cells((size_t)g.ncell), 0, false};
  int sparse = 0;
  const int64_t n = res_host_choose(h, waiting.data(), g.ncell, tile_block, sparse_fill, sparse_max, win_lo, g.ndim, g.dims, g.nonemptymgi.data(),
                                    c.want.data(), &c.holds, &sparse);
  c.want.resize((size_t)n);
  c.sparse = sparse != 0;
  return c;
}
int assign(void *h, const Cells &want, Cells &fresh) {
  fresh.assign(want.size() + 1, 0);
  int64_t n = 0;
  const int rc = res_host_assign(h, want.data(), (int64_t)want.size(), fresh.data(), &n);
  fresh.resize((size_t)n);
  return rc;
}
Cells rows(void *h, int ncell, int nrows) {
  Cells krow((size_t)ncell), rowcell((size_t)nrows);
  res_host_tables(h, krow.data(), rowcell.data());
  return rowcell;
}
}  // namespace

int main() {
  const Grid line9(1, 10, 1, 1, {4});
  const Grid grids[3] = {Grid(1, 9, 1, 1, {3, 8}), Grid(2, 4, 5, 1, {0, 6, 19}), Grid(3, 4, 4, 4, {0, 3, 21, 22, 42, 63})};
  {  // window choice: 3 rows of 9 cells
    void *h = res_host_new(9, 3);
    CHECK(choose(h, line9, {0, 1, 0, 2, 5, 4, 0, 1, 0}, 0, false).want == Cells({3, 4, 5}));
    CHECK(choose(h, line9, {0, 4, 3, 0, 0, 3, 4, 0, 0}, 0, false).want == Cells({0, 1, 2}));
    CHECK(choose(h, line9, {0, 0, 0, 0, 0, 0, 0, 0, 9}, 0, false).want == Cells({6, 7, 8}));
    CHECK(choose(h, line9, {0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, false).want == Cells({0, 1, 2}));
    CHECK(choose(h, line9, {9, 9, 9, 0, 1, 0, 0, 0, 2}, 0, false, 16384, 6).holds == 2);
    CHECK(choose(h, line9, {0, 1, 0, 2, 5, 4, 0, 1, 0}, 3, false).want == Cells({3, 4, 5}));
    res_host_free(h);
  }
  {  // block choice: blocks of 2, 5 rows
    void *h = res_host_new(9, 5);
    CHECK(choose(h, line9, {1, 0, 0, 7, 2, 2, 3, 3, 1}, 2, false).want == Cells({2, 3, 6, 7}));
    CHECK(choose(h, line9, {1, 0, 0, 7, 3, 2, 3, 3, 4}, 2, false).want == Cells({2, 3, 6, 7}));
    CHECK(choose(h, line9, {0, 0, 0, 7, 0, 0, 3, 3, 6}, 2, false).holds == 19);
    CHECK(choose(h, line9, {3, 0, 0, 0, 3, 0, 0, 0, 0}, 2, false).want == Cells({0, 1, 4, 5}));
    CHECK(choose(h, line9, {0, 0, 0, 0, 0, 0, 0, 0, 0}, 2, false).want.empty());
    res_host_free(h);
  }
  for (const Grid &g : grids) {  // sparse choice: every cell alone, at every number of rows; then choices and assignments in turn on one table
    for (int c = 0; c < g.ncell; c++) {
      Cells waiting((size_t)g.ncell, 0);
      waiting[(size_t)c] = 5;
      int taken = 0;
      for (int nrows = 1; nrows <= g.ncell + 2; nrows++) {
        void *h = res_host_new(g.ncell, nrows);
        const Choice ch = choose(h, g, waiting);
        CHECK(ch.holds == 5 && (int)ch.want.size() <= nrows);
        CHECK(ch.sparse >= (taken != 0));  // (once there are rows enough for the sparse choice, more rows do not undo it)
        taken += ch.sparse;
        CHECK(!choose(h, g, waiting, 0, true, 4).sparse && !choose(h, g, waiting, 0, false).sparse);
        res_host_free(h);
      }
    }
    void *h = res_host_new(g.ncell, g.ncell - 1);
    Cells a((size_t)g.ncell, 0), b((size_t)g.ncell, 0), fresh;
    a[0] = 3;
    b[2] = 4;
    for (const Cells *w : {&a, &a, &b, &a, &b, &b, &a}) {
      const Choice ch = choose(h, g, *w);
      CHECK(ch.sparse);
      CHECK(assign(h, ch.want, fresh) == 0);
      CHECK(choose(h, g, *w).want == ch.want);
    }
    res_host_free(h);
  }
  {  // row assignment: five wanted sets over 4 rows, the errors, a fill given back
    void *h = res_host_new(9, 4);
    Cells fresh;
    for (const Cells &want : {Cells{0, 1, 2}, Cells{2, 3}, Cells{5, 4, 2}, Cells{5, 6, 7, 8}, Cells{0}}) CHECK(assign(h, want, fresh) == 0);
    CHECK(rows(h, 9, 4) == Cells({0, 6, 7, 8}));
    CHECK(assign(h, {1, 2, 3, 4, 5}, fresh) != 0 && fresh.empty());
    CHECK(rows(h, 9, 4) == Cells({0, 6, 7, 8}));
    res_host_reset(h);
    CHECK(rows(h, 9, 4) == Cells({-1, -1, -1, -1}));
    CHECK(assign(h, {0, 1, 2, 3}, fresh) == 0 && assign(h, {4, 5, 2}, fresh) == 0 && fresh == Cells({4, 5}));
    res_host_give_back(h, fresh.data(), (int64_t)fresh.size());
    CHECK(rows(h, 9, 4) == Cells({-1, -1, 2, 3}));
    CHECK(assign(h, {7}, fresh) == 0 && rows(h, 9, 4) == Cells({7, -1, 2, 3}));
    res_host_free(h);
  }
  printf("replay ok\n");
  return 0;
}
