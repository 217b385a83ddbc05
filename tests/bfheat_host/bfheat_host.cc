// bfheat_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The bodies of artis_amd/csrc/bf_heating.h -- the ones the engine's kernels call -- compiled for x86 with g++ and applied in plain loops
// (cells split over a few std::threads) to host copies of the inputs: what artis_amd_bfheating_update computes on the device. Also exports
// tb_expm1, gk61_integrate on the analytic integrands of the golden file, and the integral of the stage's integrand over one table for
// tests/test_bfheating_rules.py.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/model_build.h"
#include "../../artis_amd/csrc/bf_heating.h"

using artis::DevModel;

namespace {
struct HostModel {
  artis::ModelOwned own;
  DevModel M;
  std::vector<int32_t> gci, levels;
  explicit HostModel(const artis_model *m) {
    M = artis::make_host_model_view(*m, own);
    gci.assign((size_t)M.nions + 1, -1);
    for (int ui = 0; ui < M.nions; ui++) {  // the ground-continuum indices, as artis_ib::alpha_sp_entry leaves them
      const artis_ib::IonOf k = artis_ib::ion_of(M, ui);
      gci[(size_t)ui] = artis_ib::ion_groundcontindex(M, k.element, k.ion);
    }
    for (int ul = 0; ul < M.nlevels; ul++)
      if (M.level_nphixstargets[ul] > 0) levels.push_back(ul);
  }
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

// the pointers of a call, in the order tests/bfheat_common.py packs them
enum Ptr { P_RES_TR, P_RES_W, P_LEV_TR, P_LEV_W, P_FIT_FLAGS, P_BFH_RAW, P_ASSOCVOL, P_MASSFRAC, P_OUT_RENORM, P_OUT_COEFFS, P_OUT_FLAGS, P_OUT_TOTALS, P_COUNT };

artis_bfh::Arrays arrays_of(const HostModel &hm, void *const *p, const double *d, const int32_t *iv) {
  artis_bfh::Arrays a{};
  const DevModel &M = hm.M;
  a.ncell = M.npts_nonempty;
  a.nbfg = M.nbfcontinua_ground;
  a.res_TR = (const float *)p[P_RES_TR];
  a.res_W = (const float *)p[P_RES_W];
  a.lev_TR = (const float *)p[P_LEV_TR];
  a.lev_W = (const float *)p[P_LEV_W];
  a.fit_flags = (const int32_t *)p[P_FIT_FLAGS];
  a.bfh_raw = (const double *)p[P_BFH_RAW];
  a.bfh_stride = 1;
  a.assocvol = (const double *)p[P_ASSOCVOL];
  a.prev_mid = d[0];
  a.tmin = d[1];
  a.deltat = d[2];
  a.nprocs = iv[0];
  a.gci = hm.gci.data();
  a.massfrac = ARTIS_OPT_USE_ION_BFHEATING_ESTIMATORS ? nullptr : (const float *)p[P_MASSFRAC];
  a.levels = hm.levels.data();
  a.nlevels_listed = (int32_t)hm.levels.size();
  a.renorm = (double *)p[P_OUT_RENORM];
  a.coeffs = (double *)p[P_OUT_COEFFS];
  a.flags = (int32_t *)p[P_OUT_FLAGS];
  return a;
}

// a DevModel that holds what artis::phixs_fromtable reads, for an integrand over a table alone
DevModel table_model(int npoints, double increment) {
  DevModel M{};
  M.NPHIXSPOINTS = npoints;
  M.NPHIXSNUINCREMENT = increment;
  M.last_phixs_nuovernuedge = (1.0 + (increment * (npoints - 1)));
  return M;
}
}  // namespace

extern "C" {

void *bfh_host_model_new(const artis_model *m) { return new HostModel(m); }
void bfh_host_model_free(void *h) { delete static_cast<HostModel *>(h); }
int bfh_host_supported(void) { return ARTIS_TB_SUPPORTED; }
int bfh_host_nptrs(void) { return P_COUNT; }
int bfh_host_nlevels_listed(const void *h) { return (int)static_cast<const HostModel *>(h)->levels.size(); }
void bfh_host_gci(const void *h, int32_t *gci) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  for (int ui = 0; ui < hm.M.nions; ui++) gci[ui] = hm.gci[(size_t)ui];
}
double bfh_host_expm1(double x) { return artis_tb::tb_expm1(x); }

// gk61_integrate on the analytic integrands (artis_amd_debug_gk61 on x86)
void bfh_host_gk61(int32_t ncases, const artis_gk61_case *cases, artis_gk61_result *out) {
  for (int32_t i = 0; i < ncases; i++) {
    int64_t evals = 0;
    const artis_bfh::Gk61TestFn f{cases[i].which, cases[i].p, &evals};
    artis_bfh::Gk61Stats st;
    double error = 0.;
    out[i].result = artis_bfh::gk61_integrate(f, cases[i].a, cases[i].b, cases[i].tol, &error, &st);
    out[i].error = error;
    out[i].evals = evals;
    out[i].nodes = st.nodes;
    out[i].maxdepth = st.maxdepth;
  }
}

// the integral of the stage's integrand over [nu_edge, nu_edge x last_phixs_nuovernuedge] for the table xs[npoints]: out = {result, error,
// nodes, maxdepth}
void bfh_host_integral(int npoints, double increment, const float *xs, double nu_edge, float T_R, float W, double *out) {
  const DevModel M = table_model(npoints, increment);
  const artis_bfh::BfhIntegrand<artis_bfh::TbMath> f = artis_bfh::bfh_integrand<artis_bfh::TbMath>(M, xs, nu_edge, T_R, W);
  artis_bfh::Gk61Stats st;
  double error = 0.;
  out[0] = artis_bfh::gk61_integrate(f, nu_edge, nu_edge * M.last_phixs_nuovernuedge, artis_bfh::EPSREL, &error, &st);
  out[1] = error;
  out[2] = st.nodes;
  out[3] = st.maxdepth;
}

// artis_amd_bfheating_update on host arrays: d = {prev_mid, tmin, deltat}, iv = {nprocs}; p[P_OUT_TOTALS]: int64 [NTOTALS]
void bfh_host_update(const void *h, void *const *p, const double *d, const int32_t *iv, int nthreads) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  const artis_bfh::Arrays a = arrays_of(hm, p, d, iv);
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<artis_bfh::Totals> tots((size_t)nt, artis_bfh::Totals{});
  parallel_cells(a.ncell, nt, [&](int t, int64_t c0, int64_t c1) {
    artis_bfh::Totals &tot = tots[(size_t)t];
    for (int64_t c = c0; c < c1; c++) {
      a.flags[c] = 0;
      for (int ul = 0; ul < M.nlevels; ul++) a.coeffs[c * M.nlevels + ul] = 0.;
      for (int g = 0; g < a.nbfg; g++) a.flags[c] |= artis_bfh::ground_cell_entry(M, a, c, g, &tot);
      if (!artis_bfh::cell_fitted(a, c)) continue;
      for (int k = 0; k < a.nlevels_listed; k++) a.flags[c] |= artis_bfh::level_cell_entry(M, a, c, k, &tot);
    }
  });
  int64_t *totals = (int64_t *)p[P_OUT_TOTALS];
  for (int k = 0; k < artis_bfh::NTOTALS; k++) {
    totals[k] = 0;
    for (const artis_bfh::Totals &t : tots) totals[k] += t.v[k];
  }
}

}  // extern "C"
