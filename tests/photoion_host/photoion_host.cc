// photoion_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The bodies of artis_amd/csrc/photoion.h -- the ones the engine's kernel calls -- compiled for x86 with g++ and applied in plain loops
// (cells split over std::threads) to host copies of a cell state: what artis_amd_set_cellstate_photoion computes on the device. Built with
// BOTH Math policies: the stage's own exp and expm1 (math = 0: the device's bits) and libm's (math = 1: the reference's arithmetic).
// Also exports the continua with their entries and estimator indices, and Tepow, for tests/test_photoion_rules.py.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/model_build.h"
#include "../../artis_amd/csrc/photoion.h"

using artis::DevModel;

namespace {
// libm's exp and expm1: what the reference's integrand calls
struct LibmMath {
  static double exp(const double x) { return std::exp(x); }
  static double expm1(const double x) { return std::expm1(x); }
};

struct HostModel {
  artis::ModelOwned own;
  DevModel M;
  explicit HostModel(const artis_model *m) { M = artis::make_host_model_view(*m, own); }
};

template <class F>
void parallel_cells(int64_t ncell, int nthreads, F work) {
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<std::thread> pool;
  const int64_t chunk = (ncell + nt - 1) / nt;
  for (int t = 0; t < nt; t++) {
    const int64_t c0 = t * chunk, c1 = c0 + chunk < ncell ? c0 + chunk : ncell;
    if (c0 < c1) pool.emplace_back(work, t, c0, c1);
  }
  for (auto &th : pool) th.join();
}

// the pointers of a call, in the order tests/photoion_common.py packs them
enum Ptr { P_TE, P_NNE, P_CLUMP, P_TR, P_W, P_LEVELPOPS, P_BIN_W, P_BIN_TR, P_BFRATE, P_OUT_COEFF, P_OUT_SOURCE, P_OUT_FLAGS, P_OUT_TOTALS, P_COUNT };

template <class Math>
void compute(const HostModel &hm, const artis_pi::Arrays &a, int nthreads, int64_t *totals) {
  const DevModel &M = hm.M;
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<artis_pi::Totals> tots((size_t)nt, artis_pi::Totals{});
  parallel_cells(a.ncell, nt, [&](int t, int64_t c0, int64_t c1) {
    artis_pi::Totals &tot = tots[(size_t)t];
    std::vector<artis_pi::BinWT> bins((size_t)artis_pi::NBINS);
    for (int64_t c = c0; c < c1; c++) {
      a.flags[c] = 0;
      for (int k = 0; k < a.nentries; k++) {
        a.coeff[c * a.nentries + k] = 0.;
        a.source[c * a.nentries + k] = artis_pi::SRC_NONE;
      }
      if (ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON && a.binned)
        for (int b = 0; b < artis_pi::NBINS; b++) artis_pi::stage_bin(a, c, b, bins.data());
      const artis_pi::CellIn cell = artis_pi::cell_in(M, a, c);
      const artis_pi::CellRadfield<Math> J = artis_pi::cell_radfield<Math>(a, c, bins.data());
      for (int i = 0; i < a.ncont; i++) a.flags[c] |= artis_pi::cont_cell_entry<Math>(M, a, c, i, cell, J, &tot);
    }
  });
  for (int k = 0; k < artis_pi::NTOTALS; k++) {
    totals[k] = 0;
    for (const artis_pi::Totals &t : tots) totals[k] += t.v[k];
  }
}
}  // namespace

extern "C" {

void *pi_host_model_new(const artis_model *m) { return new HostModel(m); }
void pi_host_model_free(void *h) { delete static_cast<HostModel *>(h); }
int pi_host_nptrs(void) { return P_COUNT; }
// out = {npts_nonempty, nphixstargets_total, nbfcontinua, nbfestim (0 without the estimators), nlevels, RADFIELDBINCOUNT,
//        MULTIBIN_RADFIELD_MODEL_ON, DETAILED_BF_ESTIMATORS_ON, FIRST_NLTE_RADFIELD_TIMESTEP, USE_LUT_PHOTOION}
void pi_host_sizes(const void *h, int64_t *out) {
  const DevModel &M = static_cast<const HostModel *>(h)->M;
  out[0] = M.npts_nonempty;
  out[1] = M.nphixstargets_total;
  out[2] = M.nbfcontinua;
  out[3] = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? M.nbfestim : 0;
  out[4] = M.nlevels;
  out[5] = artis_pi::NBINS;
  out[6] = ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON;
  out[7] = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON;
  out[8] = ARTIS_OPT_FIRST_NLTE_RADFIELD_TIMESTEP;
  out[9] = ARTIS_OPT_USE_LUT_PHOTOION;
}
// [nbfcontinua][4] {level, target, entry of the cell's row, estimator index (-1: none)} of every continuum
void pi_host_conts(const void *h, int32_t *out) {
  const DevModel &M = static_cast<const HostModel *>(h)->M;
  for (int i = 0; i < M.nbfcontinua; i++) {
    const int ul = M.allcont_uniquelevelindex[i], t = M.allcont_phixstargetindex[i];
    out[4 * i] = ul;
    out[4 * i + 1] = t;
    out[4 * i + 2] = M.level_phixstargetstart[ul] + t;
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
    out[4 * i + 3] = artis::bfestimindex(M, i);
#else
    out[4 * i + 3] = -1;
#endif
  }
}
// the bin layout of the multibin radiation field: {RADFIELDBINS_NU_MIN, RADFIELDBINS_NU_MAX, RADFIELDBINS_T_E_SUPERBIN_NU_MAX}
void pi_host_bin_consts(double *out) {
  out[0] = ARTIS_OPT_RADFIELDBINS_NU_MIN;
  out[1] = ARTIS_OPT_RADFIELDBINS_NU_MAX;
  out[2] = ARTIS_OPT_RADFIELDBINS_T_E_SUPERBIN_NU_MAX;
}
void pi_host_tepow(const float *Te, int64_t ncell, double *Tepow) { artis_pi::make_tepow(Te, ncell, Tepow); }

// artis_amd_set_cellstate_photoion's computation on host arrays. d = {use_bf_estimators, nts, unused}; Tepow is made here as the engine
// makes it; p[P_OUT_TOTALS]: int64 [NTOTALS]
void pi_host_compute(const void *h, void *const *p, const double *d, int math, int nthreads) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  artis_pi::Arrays a{};
  a.ncell = M.npts_nonempty;
  a.ncont = M.nbfcontinua;
  a.nentries = M.nphixstargets_total;
  a.nbfestim = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? M.nbfestim : 0;
  a.use_bf_estimators = (int32_t)d[0];
  a.binned = ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON && (int32_t)d[1] >= ARTIS_OPT_FIRST_NLTE_RADFIELD_TIMESTEP;
  a.Te = (const float *)p[P_TE];
  a.nne = (const float *)p[P_NNE];
  a.clumpfactor = (const float *)p[P_CLUMP];
  a.TR = (const float *)p[P_TR];
  a.W = (const float *)p[P_W];
  a.levelpops = (const double *)p[P_LEVELPOPS];
  a.bin_W = (const float *)p[P_BIN_W];
  a.bin_T_R = (const float *)p[P_BIN_TR];
  a.bfrate_normed = (const float *)p[P_BFRATE];
  a.coeff = (double *)p[P_OUT_COEFF];
  a.source = (uint8_t *)p[P_OUT_SOURCE];
  a.flags = (int32_t *)p[P_OUT_FLAGS];
  std::vector<double> Tepow((size_t)(a.ncell > 0 ? a.ncell : 1));
  artis_pi::make_tepow(a.Te, a.ncell, Tepow.data());
  a.Tepow = Tepow.data();
  if (math == 0)
    compute<artis_pi::TbMath>(hm, a, nthreads, (int64_t *)p[P_OUT_TOTALS]);
  else
    compute<LibmMath>(hm, a, nthreads, (int64_t *)p[P_OUT_TOTALS]);
}

}  // extern "C"
