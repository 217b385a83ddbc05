// radfield_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The per-element bodies of artis_amd/csrc/radfield_fit.h -- the ones the engine's kernels call -- compiled for x86 with g++ and
// applied in plain loops (cells split over a few std::threads) to host copies of the estimators and the cell state: what
// artis_amd_radfield_fit computes on the device. Also exports the pieces (Planck integrals, mean frequency, TOMS 748 on the bin residual and on a few
// analytic functions) for tests/test_radfield_fit_rules.py and tests/golden/make_toms748_golden.py.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/radfield_fit.h"

using namespace artis_rf;

namespace {
// the analytic test functions of the root finder (tests/golden/toms748_golden.cc has the same list)
double analytic(int which, double x) {
  switch (which) {
    case 0: return cos(x) - x;
    case 1: return x * x * x - 2 * x - 5;
    case 2: return exp(x) - 2;
    case 3: return x * x * x * x * x - 1e-3;
    case 4: return tanh(10 * (x - 0.3));
    default: return (x - 1) * (x - 1) * (x - 1);
  }
}
}  // namespace

extern "C" {

int rf_host_nbins(void) { return ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON ? NBINS : 0; }
double rf_host_mintemp(void) { return ARTIS_OPT_MINTEMP; }
double rf_host_maxtemp(void) { return ARTIS_OPT_MAXTEMP; }
void rf_host_bin_edges(double *lower, double *upper) {
  for (int b = 0; b < NBINS; b++) {
    lower[b] = bin_nu_lower(b);
    upper[b] = bin_nu_upper(b);
  }
}
double rf_host_partial(double x, int times_nu) {
  return times_nu ? partial_nu_planck_integral_x_to_inf(x, 1e-15) : partial_planck_integral_x_to_inf(x, 1e-15);
}
double rf_host_planck_integral(double T, double nu_low, double nu_high, int times_nu) {
  return calculate_planck_integral(T, nu_low, nu_high, times_nu != 0);
}
double rf_host_mean_frequency(double T, double nu_low, double nu_high) { return calculate_planck_mean_frequency(T, nu_low, nu_high); }
// both branches of the mean frequency, whatever x_low is: the Wien-tail form and the ratio of the series
double rf_host_mean_frequency_tail(double T, double nu_low, double nu_high) {
  const double x_low = (H * nu_low) / (KB * T);
  const double x_high = (H * nu_high) / (KB * T);
  return (KB * T / H) * (wien_tail_bin_moment(x_low, x_high, 4) / wien_tail_bin_moment(x_low, x_high, 3));
}
double rf_host_mean_frequency_series(double T, double nu_low, double nu_high) {
  return calculate_planck_integral(T, nu_low, nu_high, true) / calculate_planck_integral(T, nu_low, nu_high, false);
}

// TOMS 748 on the bin residual over [ax, bx] (out: lo, hi; returns the evaluations)
int rf_host_toms748_bin(double nu_lower, double nu_upper, double nu_bar, double ax, double bx, double tol, int maxit, double *out) {
  const BinResidual f{nu_lower, nu_upper, nu_bar};
  int evals = maxit;
  const RootPair r = toms748(f, ax, bx, f(ax), f(bx), RelTol{tol}, &evals);
  out[0] = r.lo;
  out[1] = r.hi;
  return evals;
}
int rf_host_toms748_analytic(int which, double ax, double bx, double tol, int maxit, double *out) {
  auto f = [which](double x) { return analytic(which, x); };
  int evals = maxit;
  const RootPair r = toms748(f, ax, bx, f(ax), f(bx), RelTol{tol}, &evals);
  out[0] = r.lo;
  out[1] = r.hi;
  return evals;
}
// find_bin_T_R and fit_bin as they are (bits: artis_rf::BIN_*)
float rf_host_find_bin_T_R(double nu_lower, double nu_upper, double nu_bar, int *bits, int *evals) {
  *bits = 0;
  return find_bin_T_R(nu_lower, nu_upper, nu_bar, bits, evals);
}
int rf_host_fit_bin(double J_raw, double nuJ_raw, double J_normfactor, int b, float T_e, float *T_R, float *W) {
  return fit_bin(J_raw, nuJ_raw, J_normfactor, b, T_e, T_R, W);
}

// artis_amd_radfield_fit on host arrays. est: J, nuJ [ncell]; radfieldbin_J / _nuJ [ncell * nbins] (separate arrays, as
// artis_amd_estimators_download gives them); bfrate_raw [ncell * nbf]; Jb_lu_raw / _contribcount [ncell * nline]. bf_state:
// the bound-free block the fit leaves THICK cells alone in (the engine's result block); copied to out->bfrate_normed.
void rf_host_fit(const artis_radfield_config *cfg, double tmin, int64_t ncell, int nbf, int nline, const artis_cellstate *cs,
                 const artis_estimators *est, float *bf_state, artis_radfield *out, int nthreads) {
  const int nb = rf_host_nbins();
  const int32_t lte = cfg->lte_iteration != 0;
  const CellArrays cell{out->J, out->nuJ, out->J_normfactor, out->TJ, out->TR, out->Te, out->W, out->flags, out->cell_counts};
  auto work = [&](int64_t c0, int64_t c1) {
    for (int64_t c = c0; c < c1; c++) {
      const int32_t thick = cs->thick[c];
      fit_cell_store(c, CellIn{est->J[c], est->nuJ[c], cfg->assocvolume_tmin[c], cfg->prev_mid, tmin, cfg->deltat, cfg->nprocs, lte, thick,
                               cs->TJ[c], cs->TR[c], cs->Te[c], cs->W[c]},
                     cell);
      double estimator_normfactor, over4pi;
      cell_normfactors(cfg->assocvolume_tmin[c], cfg->prev_mid, tmin, cfg->deltat, cfg->nprocs, &estimator_normfactor, &over4pi);
      if (cell_bins_carried_over(lte, thick))
        for (int b = 0; b < nb; b++) carry_bin(c * nb + b, cs->radfieldbin_T_R, cs->radfieldbin_W, out->radfieldbin_T_R, out->radfieldbin_W);
      if (cell_bf_rewritten(lte, thick))
        for (int k = 0; k < nbf; k++) bf_entry(c * nbf + k, est->bfrate_raw, estimator_normfactor, bf_state);
      for (int k = 0; k < nline; k++)
        line_entry(c * nline + k, est->Jb_lu_raw, est->Jb_lu_contribcount, over4pi, out->Jb_lu_normed, out->Jb_lu_contribcount);
      for (int b = 0; b < nb; b++) {
        const int64_t i = c * nb + b;
        const int bits = fit_bin_store(i, &est->radfieldbin_J[i], &est->radfieldbin_nuJ[i], out->flags, out->J_normfactor, cs->Te,
                                       out->radfieldbin_T_R, out->radfieldbin_W);
        for (int k = 0; k < ARTIS_RADFIELD_NCOUNTS; k++) out->cell_counts[c * ARTIS_RADFIELD_NCOUNTS + k] += (bits >> k) & 1;
      }
    }
  };
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<std::thread> pool;
  const int64_t chunk = (ncell + nt - 1) / nt;
  for (int t = 0; t < nt; t++) {
    const int64_t c0 = t * chunk, c1 = c0 + chunk < ncell ? c0 + chunk : ncell;
    if (c0 < c1) pool.emplace_back(work, c0, c1);
  }
  for (auto &th : pool) th.join();
  if (nbf > 0 && out->bfrate_normed) std::memcpy(out->bfrate_normed, bf_state, sizeof(float) * (size_t)(ncell * nbf));
  for (int k = 0; k < ARTIS_RADFIELD_NCOUNTS; k++) {
    out->totals[k] = 0;
    for (int64_t c = 0; c < ncell; c++) out->totals[k] += out->cell_counts[c * ARTIS_RADFIELD_NCOUNTS + k];
  }
  out->npts_nonempty = (int32_t)ncell;
  out->nbins = nb;
  out->nbfestim = nbf;
  out->detailed_linecount = nline;
}

}  // extern "C"
