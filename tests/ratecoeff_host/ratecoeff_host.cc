// ratecoeff_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The bodies of artis_amd/csrc/ratecoeff_tables.h -- the ones the engine's kernel calls -- compiled for x86 with g++ and applied in plain
// loops (items split over std::threads): what artis_amd_ratecoeff_compute computes on the device. Built with BOTH Math policies: the
// stage's own exp and expm1 (math = 0: the device's bits) and libm's (math = 1: the reference's arithmetic), and in both forms: alpha_sp
// and bfcooling from shared evaluations (shared = 1: the kernel's) or three independent gk61_integrate calls per entry (shared = 0).
// Also exports the GK61 tables, the temperature grid and Tpow it uses for tests/test_ratecoeff_rules.py.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/model_build.h"
#include "../../artis_amd/csrc/ratecoeff_tables.h"

using artis::DevModel;

namespace {
// libm's exp and expm1: what the reference's integrands call
struct LibmMath {
  static double exp(const double x) { return std::exp(x); }
  static double expm1(const double x) { return std::expm1(x); }
};

struct HostModel {
  artis::ModelOwned own;
  DevModel M;
  std::vector<artis_rc::Cont> conts;
  std::vector<double> Tpow;
  int64_t ncovered = 0;
  bool listed = false;
  explicit HostModel(const artis_model *m) {
    M = artis::make_host_model_view(*m, own);
    listed = artis_rc::list_continua(M.nelements, M.nbfcontinua, m->nphixslevels, M.elem_nions, M.elem_uniqueionindexstart, M.ion_nlevels_ionising,
                                     M.ion_uniquelevelindexstart, M.level_nphixstargets, M.level_bflist_start, M.level_phixsstart, conts);
    for (const artis_rc::Cont &c : conts) ncovered += c.ul >= 0;
    Tpow.resize(artis_rc::TABLESIZE);
    artis_rc::make_tpow(M.temperature_grid, Tpow.data());
  }
};

template <class F>
void parallel_items(int64_t n, int nthreads, F work) {
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<std::thread> pool;
  const int64_t chunk = (n + nt - 1) / nt;
  for (int t = 0; t < nt; t++) {
    const int64_t i0 = t * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
    if (i0 < i1) pool.emplace_back(work, t, i0, i1);
  }
  for (auto &th : pool) th.join();
}

template <class Math>
void tables(const HostModel &hm, const artis_rc::Arrays &A, bool shared, int nthreads, int64_t *totals) {
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<artis_rc::Totals> tots((size_t)nt, artis_rc::Totals{});
  parallel_items(A.nitems, nt, [&](int t, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; i++) artis_rc::item_entry<Math>(hm.M, A, i, shared, &tots[(size_t)t]);
  });
  for (int k = 0; k < artis_rc::NTOTALS; k++) {
    totals[k] = 0;
    for (const artis_rc::Totals &t : tots) totals[k] += t.v[k];
  }
}
}  // namespace

extern "C" {

void *rc_host_model_new(const artis_model *m) { return new HostModel(m); }
void rc_host_model_free(void *h) { delete static_cast<HostModel *>(h); }
// out = {nbfcontinua, TABLESIZE, tables (3 with USE_LUT_PHOTOION, else 2), rows covered, 1 if every row lies inside the tables}
void rc_host_sizes(const void *h, int64_t *out) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  out[0] = hm.M.nbfcontinua;
  out[1] = artis_rc::TABLESIZE;
  out[2] = ARTIS_OPT_USE_LUT_PHOTOION ? 3 : 2;
  out[3] = hm.ncovered;
  out[4] = hm.listed;
}
// [nbfcontinua][2] {level, target} of every row (-1, -1: not covered)
void rc_host_conts(const void *h, int32_t *out) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  for (size_t i = 0; i < hm.conts.size(); i++) {
    out[2 * i] = hm.conts[i].ul;
    out[2 * i + 1] = hm.conts[i].t;
  }
}
void rc_host_tgrid(const void *h, double *tgrid, double *Tpow) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  for (int t = 0; t < artis_rc::TABLESIZE; t++) {
    tgrid[t] = hm.M.temperature_grid[t];
    Tpow[t] = hm.Tpow[(size_t)t];
  }
}
// the 61-point rule's constants as the integrator holds them: x[31], w[31], wg[15]
void rc_host_gk61_tables(double *x, double *w, double *wg) {
  const artis_bfh::GK61 &g = artis_bfh::gk61_tables();
  std::memcpy(x, g.x, sizeof g.x);
  std::memcpy(w, g.w, sizeof g.w);
  std::memcpy(wg, g.wg, sizeof g.wg);
}

// artis_amd_ratecoeff_compute on host arrays: spont, corrphotoion (null in builds without USE_LUT_PHOTOION), bfcooling and flags
// [nbfcontinua * TABLESIZE]; totals: int64 [4] {integrals, nodes, integrals at depth 15, flagged entries}
void rc_host_tables(const void *h, int math, int shared, int nthreads, double *spont, double *corrphotoion, double *bfcooling, int32_t *flags,
                    int64_t *totals) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  artis_rc::Arrays A{};
  A.nitems = (int64_t)hm.M.nbfcontinua * artis_rc::TABLESIZE;
  A.conts = hm.conts.data();
  A.Tpow = hm.Tpow.data();
  A.spontrecomb = spont;
  A.corrphotoion = ARTIS_OPT_USE_LUT_PHOTOION ? corrphotoion : nullptr;
  A.bfcooling = bfcooling;
  A.flags = flags;
  if (math == 0)
    tables<artis_rc::TbMath>(hm, A, shared != 0, nthreads, totals);
  else
    tables<LibmMath>(hm, A, shared != 0, nthreads, totals);
}

}  // extern "C"
