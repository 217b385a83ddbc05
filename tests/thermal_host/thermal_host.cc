// thermal_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The bodies of artis_amd/csrc/thermal_balance.h -- the ones the engine's kernels call -- compiled for x86 with g++ and applied in plain
// loops (cells split over a few std::threads, the 64 lanes of a wave as a loop: artis_tb::SeqLanes) to host copies of the inputs: what
// artis_amd_thermal_solve and artis_amd_thermal_rates compute on the device. Also exports the residual of one cell at given
// temperatures for tests/test_thermal_balance_rules.py.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/model_build.h"
#include "../../artis_amd/csrc/thermal_balance.h"

using artis::DevModel;

namespace {
struct HostModel {
  artis::ModelOwned own;
  DevModel M;
  std::vector<float> alpha_sp;
  std::vector<int32_t> gci, target_level;
  explicit HostModel(const artis_model *m) {
    M = artis::make_host_model_view(*m, own);
    alpha_sp.assign((size_t)M.nions * ARTIS_OPT_TABLESIZE + 1, 0.f);
    gci.assign((size_t)M.nions + 1, -1);
    for (int ui = 0; ui < M.nions; ui++)
      for (int t = 0; t < ARTIS_OPT_TABLESIZE; t++) artis_ib::alpha_sp_entry(M, ui, t, alpha_sp.data(), gci.data());
    target_level.assign((size_t)M.nphixstargets_total + 1, 0);
    for (int ul = 0; ul < M.nlevels; ul++)
      for (int t = 0; t < M.level_nphixstargets[ul]; t++) target_level[(size_t)(M.level_phixstargetstart[ul] + t)] = ul;
  }
};

template <class F>
void parallel_cells(int64_t ncell, int nthreads, F work) {
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<std::thread> pool;
  const int64_t chunk = (ncell + nt - 1) / nt;
  for (int t = 0; t < nt; t++) {
    const int64_t c0 = t * chunk, c1 = c0 + chunk < ncell ? c0 + chunk : ncell;
    if (c0 < c1) pool.emplace_back(work, c0, c1);
  }
  for (auto &th : pool) th.join();
}

// the pointers of a call, in the order tests/thermal_common.py packs them
enum Ptr {
  P_RES_TJ, P_RES_TR, P_RES_W, P_RES_TE, P_RES_NNE, P_RES_GROUND, P_RES_U, P_RES_RENORM, P_FIT_TJ, P_FIT_FLAGS, P_FIT_TE, P_RHO, P_MASSFRAC,
  P_MEANWEIGHT, P_CLUMP, P_GAMMA_RAW, P_FF_RAW, P_COL_RAW, P_ASSOCVOL, P_BFHEAT, P_NTLEPTON, P_DEP_ALPHA, P_DEP_SPFISSION,
  P_OUT_RENORM, P_OUT_GAMMA, P_OUT_U, P_OUT_TE, P_OUT_NNE, P_OUT_TE_SOLVED, P_OUT_BRACKET, P_OUT_EVALS, P_OUT_FLAGS, P_OUT_RATES,
  P_OUT_GROUND, P_OUT_PHI, P_RATES_TE, P_COUNT
};

artis_tb::Arrays arrays_of(const HostModel &hm, void *const *p, const double *d, const int32_t *iv) {
  artis_tb::Arrays a{};
  const DevModel &M = hm.M;
  a.ncell = M.npts_nonempty;
  a.nbfg = M.nbfcontinua_ground;
  a.res_TJ = (const float *)p[P_RES_TJ];
  a.res_TR = (const float *)p[P_RES_TR];
  a.res_W = (const float *)p[P_RES_W];
  a.res_Te = (const float *)p[P_RES_TE];
  a.res_nne = (const float *)p[P_RES_NNE];
  a.res_ground = (const float *)p[P_RES_GROUND];
  a.res_U = (const float *)p[P_RES_U];
  a.res_renorm = (const double *)p[P_RES_RENORM];
  a.fit_TJ = (const float *)p[P_FIT_TJ];
  a.fit_flags = (const int32_t *)p[P_FIT_FLAGS];
  a.rho = (const float *)p[P_RHO];
  a.massfrac = (const float *)p[P_MASSFRAC];
  a.meanweight_cell = (const float *)p[P_MEANWEIGHT];
  a.meanweight_model = M.elem_meannucmass;
  a.clump = (const float *)p[P_CLUMP];
  a.gamma_raw = (const double *)p[P_GAMMA_RAW];
  a.ff_raw = (const double *)p[P_FF_RAW];
  a.col_raw = (const double *)p[P_COL_RAW];
  a.gamma_stride = 1;
  a.est_stride = 1;
  a.assocvol = (const double *)p[P_ASSOCVOL];
  a.prev_mid = d[0];
  a.tmin = d[1];
  a.deltat = d[2];
  a.nprocs = iv[0];
  a.bfheatingcoeffs = (const double *)p[P_BFHEAT];
  a.ntlepton_dep = (const double *)p[P_NTLEPTON];
  a.dep_alpha = (const double *)p[P_DEP_ALPHA];
  a.dep_spfission = (const double *)p[P_DEP_SPFISSION];
  a.alpha_sp = hm.alpha_sp.data();
  a.gci = hm.gci.data();
  a.target_level = hm.target_level.data();
  a.renorm = (double *)p[P_OUT_RENORM];
  a.gamma = (double *)p[P_OUT_GAMMA];
  a.U = (float *)p[P_OUT_U];
  a.Te = (float *)p[P_OUT_TE];
  a.nne = (float *)p[P_OUT_NNE];
  a.Te_solved = (double *)p[P_OUT_TE_SOLVED];
  a.bracket = (double *)p[P_OUT_BRACKET];
  a.evals = (int32_t *)p[P_OUT_EVALS];
  a.flags = (int32_t *)p[P_OUT_FLAGS];
  a.rates = (double *)p[P_OUT_RATES];
  a.ground = (float *)p[P_OUT_GROUND];
  a.phi = (double *)p[P_OUT_PHI];
  return a;
}

// a "wave's" private rows of one cell
struct Rows {
  std::vector<double> phi, e_l;
  std::vector<float> ground;
  std::vector<int32_t> uppermost;
  explicit Rows(const DevModel &M) : phi((size_t)M.nions + 1), e_l((size_t)M.nlevels + 1), ground((size_t)M.nions + 1), uppermost((size_t)M.nelements + 1) {}
  artis_tb::CellWork work(const artis_tb::Arrays &a, const DevModel &M, int64_t c) {
    for (int ui = 0; ui < M.nions; ui++) {
      ground[(size_t)ui] = a.res_ground[c * M.nions + ui];
      phi[(size_t)ui] = 0.;
    }
    artis_tb::CellWork w{};
    w.phi = phi.data();
    w.ground = ground.data();
    w.uppermost = uppermost.data();
    w.nne = a.res_nne[c];
    return w;
  }
};
}  // namespace

extern "C" {

void *tb_host_model_new(const artis_model *m) { return new HostModel(m); }
void tb_host_model_free(void *h) { delete static_cast<HostModel *>(h); }
int tb_host_supported(void) { return ARTIS_TB_SUPPORTED; }
double tb_host_accuracy(void) { return artis_tb::ACCURACY; }
double tb_host_mintemp(void) { return artis_tb::MINTEMP; }
double tb_host_maxtemp(void) { return artis_tb::MAXTEMP; }
int tb_host_nptrs(void) { return P_COUNT; }
void tb_host_gci(const void *h, int32_t *gci) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  for (int ui = 0; ui < hm.M.nions; ui++) gci[ui] = hm.gci[(size_t)ui];
}
double tb_host_exp(double x) { return artis_tb::tb_exp(x); }
double tb_host_log(double x) { return artis_tb::tb_log(x); }
// the largest relative difference between the stage's tb_col_exc / tb_col_ion and physics.h's col_exc / col_ion over every upward
// transition (out[0]) and every ionising photoionisation target (out[1]) at T_e, cnne; out[2]: how many were compared
void tb_host_ratecoeff_diff(const void *h, float T_e, float cnne, double *out) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  out[0] = out[1] = out[2] = 0.;
  const auto rel = [](double a, double b) { return a == b ? 0. : std::fabs(a - b) / std::fabs(b); };
  for (int ati = 0; ati < M.nalltrans; ati++) {
    const int ul = M.alltrans_owner[ati];
    if (ati - M.level_alltrans_startdown[ul] < M.level_ndowntrans[ul]) continue;
    const int tul = M.ion_uniquelevelindexstart[M.level_ion[ul]] + M.alltrans_targetlevelindex[ati];
    const double e_trans = artis::eps(M, tul) - artis::eps(M, ul);
    const double a = artis_tb::tb_col_exc(M, T_e, cnne, e_trans, artis::statw(M, tul), artis::statw(M, ul), ati);
    const double b = artis::col_exc(M, T_e, cnne, e_trans, artis::statw(M, tul), artis::statw(M, ul), ati);
    if (b > 1e-280) out[0] = std::fmax(out[0], rel(a, b));  // (below: subnormal spacing)
    out[2] += 1;
  }
  for (int k = 0; k < M.nphixstargets_total; k++) {
    const artis_tb::TargetOf o = artis_tb::target_of(M, hm.target_level.data(), k);
    if (!o.ionises) continue;
    const double e_trans = artis::eps(M, M.ion_uniquelevelindexstart[o.ui + 1] + artis::phixs_upperlevel(M, o.ul, o.t)) - artis::eps(M, o.ul);
    const double a = artis_tb::tb_col_ion(M, T_e, cnne, o.element, o.ion, o.level, o.t, e_trans);
    const double b = artis::col_ion(M, T_e, cnne, o.element, o.ion, o.level, o.t, e_trans);
    if (b > 1e-280) out[1] = std::fmax(out[1], rel(a, b));
    out[2] += 1;
  }
}
// artis_tb::combine64 of 64 doubles (in place)
double tb_host_combine64(double *p) { return artis_tb::combine64(p); }

// artis_amd_thermal_solve on host arrays: d = {prev_mid, tmin, deltat}, iv = {nprocs}
void tb_host_solve(const void *h, void *const *p, const double *d, const int32_t *iv, int nthreads) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  const artis_tb::Arrays a = arrays_of(hm, p, d, iv);
  const float *fit_Te = (const float *)p[P_FIT_TE];
  const artis_tb::SeqLanes lanes;
  parallel_cells(a.ncell, nthreads, [&](int64_t c0, int64_t c1) {
    Rows rows(M);
    for (int64_t c = c0; c < c1; c++) {
      artis_tb::cell_clear(M, a, c, fit_Te);
      for (int g = 0; g < a.nbfg; g++) a.flags[c] |= artis_tb::renorm_cell_entry(M, a, c, g);
      for (int ui = 0; ui < M.nions; ui++) artis_tb::gamma_cell_entry(M, a, c, ui);
      for (int ui = 0; ui < M.nions; ui++) artis_ib::partfunct_entry(M, c, ui, a.fit_TJ, a.fit_TJ, a.res_ground, a.massfrac, a.U, &a.flags[c]);
      if (!artis_tb::cell_fitted(a, c)) continue;
      artis_tb::fill_boltzmann(M, a.fit_TJ[c], rows.e_l.data(), lanes);
      const artis_tb::CellFixed f = artis_tb::cell_fixed(M, a, c, a.U + c * M.nions, a.gamma + c * a.nbfg, rows.e_l.data());
      artis_tb::CellWork w = rows.work(a, M, c);
      const artis_tb::Found r = artis_tb::find_Te(M, f, w, lanes);
      artis_tb::cell_store(M, a, c, r, w);
    }
  });
}

// artis_amd_thermal_rates on host arrays (p[P_RATES_TE] null: the resident T_e); rebalance = 1 reads U and gamma of an earlier
// tb_host_solve from the output arrays
void tb_host_rates(const void *h, void *const *p, const double *d, const int32_t *iv, int rebalance, int nthreads) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  const artis_tb::Arrays a = arrays_of(hm, p, d, iv);
  const float *Te = (const float *)p[P_RATES_TE];
  const artis_tb::SeqLanes lanes;
  parallel_cells(a.ncell, nthreads, [&](int64_t c0, int64_t c1) {
    Rows rows(M);
    for (int64_t c = c0; c < c1; c++) {
      artis_tb::fill_boltzmann(M, rebalance ? a.fit_TJ[c] : a.res_TJ[c], rows.e_l.data(), lanes);
      const artis_tb::CellFixed f = artis_tb::cell_fixed(M, a, c, (rebalance ? a.U : a.res_U) + c * M.nions, a.gamma + c * a.nbfg, rows.e_l.data());
      artis_tb::CellWork w = rows.work(a, M, c);
      const float T_e = Te ? Te[c] : a.res_Te[c];
      artis_tb::rates_cell(M, a, c, f, w, T_e, rebalance != 0, lanes);
      artis_tb::rates_store(M, a, c, T_e, rebalance != 0, w);
    }
  });
}

// the residual (with its ion balance) of cell c at T[0..nT) after a tb_host_solve on the same arrays (its U and gamma): out[nT]
void tb_host_residuals(const void *h, void *const *p, const double *d, const int32_t *iv, int64_t c, int nT, const double *T, double *out) {
  const HostModel &hm = *static_cast<const HostModel *>(h);
  const DevModel &M = hm.M;
  const artis_tb::Arrays a = arrays_of(hm, p, d, iv);
  const artis_tb::SeqLanes lanes;
  Rows rows(M);
  artis_tb::fill_boltzmann(M, a.fit_TJ[c], rows.e_l.data(), lanes);
  const artis_tb::CellFixed f = artis_tb::cell_fixed(M, a, c, a.U + c * M.nions, a.gamma + c * a.nbfg, rows.e_l.data());
  for (int i = 0; i < nT; i++) {
    artis_tb::CellWork w = rows.work(a, M, c);
    out[i] = artis_tb::residual(M, f, w, T[i], lanes);
  }
}

}  // extern "C"
