// radfield_fit.h -- the radiation-field fit of the grid update, per cell and per frequency bin.
//
// What the reference does to a cell's radiation-field estimators between two timesteps (update_grid_cell,
// update_grid.cc:462-573): normalise J (and, in fitted cells, nuJ), derive T_J from J alone in LTE / THICK cells
// (get_T_J_from_J radfield.cc:956), otherwise fit a diluted blackbody to the whole spectrum (set_params_fullspec) and,
// with the multibin model, one (W, T_R) per frequency bin (fit_parameters, find_bin_T_R: a bracketed TOMS 748 root of
// the Planck mean frequency minus the bin's nuJ / J). The detailed bound-free and line estimators are normalised too
// (normalise_bf_estimators radfield.cc:902-925, normalise_J :893-899). The engine's kernels (stage_radfield.h) and the loops of
// tests/radfield_host (x86) call the same per-element functions at the end of this file.
//
// Floating-point discipline as physics.h: -ffp-contract=off, and every expression keeps the reference's order of
// operations, float/double mixing included (pow4 of a float T_R is a float product, as the reference's auto template).
// The log lines of the reference become flag bits and counts (include/artis_amd.h ARTIS_RADFIELD_*).
#pragma once
#include "physics.h"

namespace artis_rf {

using artis::CLIGHT;
using artis::KB;
using artis::PI;
constexpr double H = artis::HPLANCK;
constexpr double STEBO = 5.670400e-5;  // constants.h:41
constexpr double DBL_EPS = 2.220446049250313080847e-16;
constexpr double DBL_MAXV = 1.7976931348623157e308;
constexpr double DBL_MINV = 2.2250738585072014e-308;
constexpr double BINS_T_R_MIN = 500;     // radfield.cc:45
constexpr double BINS_T_R_MAX = 250000;  // radfield.cc:46
constexpr int NBINS = ARTIS_OPT_RADFIELDBINCOUNT;
constexpr int MAXIT = 100;  // find_bin_T_R

// constants.h:16-19 (templates on the argument's type: a float stays float)
template <typename T>
AHD T rf_pow2(T x) {
  return x * x;
}
template <typename T>
AHD T rf_pow3(T x) {
  return x * x * x;
}
template <typename T>
AHD T rf_pow4(T x) {
  return rf_pow2(x) * rf_pow2(x);
}
template <typename T>
AHD T rf_pow5(T x) {
  return rf_pow4(x) * x;
}

AHD double bin_nu_upper(int b) { return artis::radbin_nu_upper(b); }
AHD double bin_nu_lower(int b) { return b > 0 ? artis::radbin_nu_upper(b - 1) : ARTIS_OPT_RADFIELDBINS_NU_MIN; }  // radfield.cc:127

// ---- Planck integrals (radfield.cc:253-338, :513-538)

// Series for the integral of x^3 / (e^x - 1) from x to infinity; stops at the first term below sum * epsrel
AHD double partial_planck_integral_x_to_inf(const double x, const double epsrel) {
  if (x > 700) return 0.0;
  double sum = 0.0;
  for (int n = 1; n < 1000; ++n) {
    const double n2 = n * n;
    const double n3 = n2 * n;
    const double n4 = n3 * n;
    const double term = exp(-n * x) * ((rf_pow3(x) / n) + (3.0 * rf_pow2(x) / n2) + (6.0 * x / n3) + (6.0 / n4));
    sum += term;
    if (term < sum * epsrel) break;
  }
  return sum;
}

// ... of x^4 / (e^x - 1)
AHD double partial_nu_planck_integral_x_to_inf(const double x, const double epsrel) {
  if (x > 700) return 0.0;
  double sum = 0.0;
  for (int n = 1; n < 1000; ++n) {
    const double n2 = n * n;
    const double n3 = n2 * n;
    const double n4 = n3 * n;
    const double n5 = n4 * n;
    const double term =
        exp(-n * x) * ((rf_pow4(x) / n) + (4.0 * rf_pow3(x) / n2) + (12.0 * rf_pow2(x) / n3) + (24.0 * x / n4) + (24.0 / n5));
    sum += term;
    if (term < sum * epsrel) break;
  }
  return sum;
}

AHD double calculate_planck_integral(const double temperature, const double nu_low, const double nu_high, const bool times_nu) {
  if (temperature <= 0) return 0.0;
  constexpr double epsrel = 1e-15;
  const double x_low = (H * nu_low) / (KB * temperature);
  const double x_high = (H * nu_high) / (KB * temperature);
  if (times_nu) {
    const double constant_factor = (2.0 * rf_pow5(KB) * rf_pow5(temperature)) / (rf_pow4(H) * rf_pow2(CLIGHT));
    const double low_to_inf = partial_nu_planck_integral_x_to_inf(x_low, epsrel);
    const double high_to_inf = partial_nu_planck_integral_x_to_inf(x_high, epsrel);
    return constant_factor * (low_to_inf - high_to_inf);
  }
  const double constant_factor = (2.0 * rf_pow4(KB) * rf_pow4(temperature)) / (rf_pow3(H) * rf_pow2(CLIGHT));
  const double low_to_inf = partial_planck_integral_x_to_inf(x_low, epsrel);
  const double high_to_inf = partial_planck_integral_x_to_inf(x_high, epsrel);
  return constant_factor * (low_to_inf - high_to_inf);
}

// Wien-tail moment of one bin with exp(-x_low) factored out (radfield.cc:313-327); deg 3: J, deg 4: nuJ
AHD double wien_tail_polynomial(const double x, const int deg) {
  if (deg == 3) return rf_pow3(x) + (3 * rf_pow2(x)) + (6 * x) + 6;
  return rf_pow4(x) + (4 * rf_pow3(x)) + (12 * rf_pow2(x)) + (24 * x) + 24;
}
AHD double wien_tail_bin_moment(const double x_low, const double x_high, const int deg) {
  const double bin_width = x_high - x_low;
  const double exp_minus_bin_width = exp(-bin_width);
  const double polynomial_low = wien_tail_polynomial(x_low, deg);
  const double polynomial_high = wien_tail_polynomial(x_high, deg);
  return (-expm1(-bin_width) * polynomial_low) - (exp_minus_bin_width * (polynomial_high - polynomial_low));
}

// intensity-weighted mean frequency of a blackbody in [nu_low, nu_high] (radfield.cc:301)
AHD double calculate_planck_mean_frequency(const double temperature, const double nu_low, const double nu_high) {
  const double x_low = (H * nu_low) / (KB * temperature);
  const double x_high = (H * nu_high) / (KB * temperature);
  constexpr double wien_tail_threshold = 100.;
  if (x_low >= wien_tail_threshold) {
    const double planck_moment = wien_tail_bin_moment(x_low, x_high, 3);
    const double nu_planck_moment = wien_tail_bin_moment(x_low, x_high, 4);
    return (KB * temperature / H) * (nu_planck_moment / planck_moment);
  }
  const double nu_planck_integral = calculate_planck_integral(temperature, nu_low, nu_high, true);
  const double planck_integral = calculate_planck_integral(temperature, nu_low, nu_high, false);
  return nu_planck_integral / planck_integral;
}

// ---- bracketing root finder: TOMS Algorithm 748 (G. E. Alefeld, F. A. Potra, Y. Shi, ACM TOMS 21 (1995) 327-344), the
// variant with one double-length secant step and a bisection when an iteration shrinks the bracket by less than half, in
// the floating-point operation order of the reference's solver (toms748.h) so that roots and evaluation counts agree bit for
// bit. Never throws: an empty or unbracketed interval gives a NaN pair, as the reference's GPU build does.

// relative bracket width (sn3d.h:77 ftol<fractional_accuracy>); the min as std::min writes it
struct RelTol {
  double frac;
  AHD bool operator()(const double a, const double b) const {
    const double fa = fabs(a), fb = fabs(b);
    return fabs(a - b) <= (frac * ((fb < fa) ? fb : fa));
  }
};

struct RootPair {
  double lo, hi;
};

namespace t748 {

AHD int sgn(const double z) { return z == 0 ? 0 : (signbit(z) ? -1 : 1); }

// num / denom, or `fallback` when the quotient would overflow
AHD double guarded_quotient(const double num, const double denom, const double fallback) {
  if (fabs(denom) < 1 && fabs(denom * DBL_MAXV) <= fabs(num)) return fallback;
  return num / denom;
}

// state of the search: [a, b] encloses the root; d, e are the points dropped most recently (third and fourth best)
struct State {
  double a, b, fa, fb, d, fd, e, fe;
};

// secant point of [a, b], or the midpoint when it falls within a few ulps of an end
AHD double secant_point(const double a, const double b, const double fa, const double fb) {
  const double rel = DBL_EPS * 5;
  const double c = a - ((fa / (fb - fa)) * (b - a));
  if ((c <= a + (fabs(a) * rel)) || (c >= b - (fabs(b) * rel))) return (a + b) / 2;
  return c;
}

// root of the quadratic through (a, fa), (b, fb), (d, fd) by `steps` Newton iterations; secant point when that fails
AHD double newton_quadratic_point(const State &s, const unsigned steps) {
  const double slope_ab = guarded_quotient(s.fb - s.fa, s.b - s.a, DBL_MAXV);
  double curv = guarded_quotient(s.fd - s.fb, s.d - s.b, DBL_MAXV);
  curv = guarded_quotient(curv - slope_ab, s.d - s.a, 0.);
  if (curv == 0) return secant_point(s.a, s.b, s.fa, s.fb);
  double x = (sgn(curv) * sgn(s.fa) > 0) ? s.a : s.b;
  for (unsigned i = 1; i <= steps; ++i) {
    const double p = s.fa + ((slope_ab + (curv * (x - s.b))) * (x - s.a));
    const double dp = slope_ab + (curv * ((2 * x) - s.a - s.b));
    x -= guarded_quotient(p, dp, 1 + x - s.a);
  }
  if ((x <= s.a) || (x >= s.b)) x = secant_point(s.a, s.b, s.fa, s.fb);
  return x;
}

// inverse cubic interpolation through (a, b, d, e); the quadratic point (3 Newton steps) when it leaves (a, b)
AHD double inverse_cubic_point(const State &s) {
  const double q11 = (s.d - s.e) * s.fd / (s.fe - s.fd);
  const double q21 = (s.b - s.d) * s.fb / (s.fd - s.fb);
  const double q31 = (s.a - s.b) * s.fa / (s.fb - s.fa);
  const double d21 = (s.b - s.d) * s.fd / (s.fd - s.fb);
  const double d31 = (s.a - s.b) * s.fb / (s.fb - s.fa);
  const double q22 = (d21 - q11) * s.fb / (s.fe - s.fb);
  const double q32 = (d31 - q21) * s.fa / (s.fd - s.fa);
  const double d32 = (d31 - q21) * s.fd / (s.fd - s.fa);
  const double q33 = (d32 - q22) * s.fa / (s.fe - s.fa);
  double x = q31 + q32 + q33 + s.a;
  if ((x <= s.a) || (x >= s.b)) x = newton_quadratic_point(s, 3);
  return x;
}

// fewer than four distinct function values: inverse cubic interpolation is ill-posed
AHD bool values_too_close(const State &s) {
  const double m = DBL_MINV * 32;
  return (fabs(s.fa - s.fb) < m) || (fabs(s.fa - s.fd) < m) || (fabs(s.fa - s.fe) < m) || (fabs(s.fb - s.fd) < m) ||
         (fabs(s.fb - s.fe) < m) || (fabs(s.fd - s.fe) < m);
}

// evaluate f at x (moved inside the bracket when within ulps of an end) and keep the half that changes sign; the
// dropped end becomes d. An exact zero collapses the bracket onto it.
template <class F>
AHD void shrink(F &f, State &s, double x) {
  const double rel = DBL_EPS * 2;
  if ((s.b - s.a) < 2 * rel * s.a) {
    x = s.a + ((s.b - s.a) / 2);
  } else if (x <= s.a + (fabs(s.a) * rel)) {
    x = s.a + (fabs(s.a) * rel);
  } else if (x >= s.b - (fabs(s.b) * rel)) {
    x = s.b - (fabs(s.b) * rel);
  }
  const double fx = f(x);
  if (fx == 0) {
    s.a = x;
    s.fa = 0;
    s.d = 0;
    s.fd = 0;
    return;
  }
  if (sgn(s.fa) * sgn(fx) < 0) {
    s.d = s.b;
    s.fd = s.fb;
    s.b = x;
    s.fb = fx;
  } else {
    s.d = s.a;
    s.fd = s.fa;
    s.a = x;
    s.fa = fx;
  }
}

}  // namespace t748

// Root of f in [ax, bx] given f(ax), f(bx) of opposite sign. On return *evals holds the evaluations used (at most the
// value it held on entry) and the final bracket is returned.
template <class F, class Tol>
AHD RootPair toms748(F f, const double ax, const double bx, const double fax, const double fbx, const Tol tol, int *evals) {
  using namespace t748;
  const int budget = *evals;
  if (budget == 0) return {ax, bx};
  const double nan = __builtin_nan("");
  if (ax >= bx) {
    *evals = 0;
    return {nan, nan};
  }
  State s{ax, bx, fax, fbx, 0., 1e5, 1e5, 1e5};
  if (tol(s.a, s.b) || (s.fa == 0) || (s.fb == 0)) {
    *evals = 0;
    if (s.fa == 0) {
      s.b = s.a;
    } else if (s.fb == 0) {
      s.a = s.b;
    }
    return {s.a, s.b};
  }
  if (sgn(s.fa) * sgn(s.fb) > 0) {
    *evals = 0;
    return {nan, nan};
  }
  int left = budget;
  auto done = [&]() { return left == 0 || s.fa == 0 || tol(s.a, s.b); };
  // first a secant step, then one quadratic step
  shrink(f, s, secant_point(s.a, s.b, s.fa, s.fb));
  --left;
  if (!done()) {
    const double x = newton_quadratic_point(s, 2);
    s.e = s.d;
    s.fe = s.fd;
    shrink(f, s, x);
    --left;
  }
  while (!done()) {
    const double width0 = s.b - s.a;
    // two interpolation steps (cubic unless the values are too close)
    double x = values_too_close(s) ? newton_quadratic_point(s, 2) : inverse_cubic_point(s);
    s.e = s.d;
    s.fe = s.fd;
    shrink(f, s, x);
    if (--left == 0 || s.fa == 0 || tol(s.a, s.b)) break;
    x = values_too_close(s) ? newton_quadratic_point(s, 3) : inverse_cubic_point(s);
    shrink(f, s, x);
    if (--left == 0 || s.fa == 0 || tol(s.a, s.b)) break;
    // a double-length secant step from the end with the smaller residual
    const bool from_a = fabs(s.fa) < fabs(s.fb);
    const double u = from_a ? s.a : s.b;
    const double fu = from_a ? s.fa : s.fb;
    x = u - (2 * (fu / (s.fb - s.fa)) * (s.b - s.a));
    if (fabs(x - u) > (s.b - s.a) / 2) x = s.a + ((s.b - s.a) / 2);
    s.e = s.d;
    s.fe = s.fd;
    shrink(f, s, x);
    if (--left == 0 || s.fa == 0 || tol(s.a, s.b)) break;
    // bisect when the iteration did not halve the bracket
    if ((s.b - s.a) < 0.5 * width0) continue;
    s.e = s.d;
    s.fe = s.fd;
    shrink(f, s, s.a + ((s.b - s.a) / 2));
    --left;
  }
  *evals = budget - left;
  if (s.fa == 0) {
    s.b = s.a;
  } else if (s.fb == 0) {
    s.a = s.b;
  }
  return {s.a, s.b};
}

// ---- one frequency bin (find_bin_T_R radfield.cc:366, fit_parameters :806-881)

// residual of the bin fit: Planck mean frequency at T_R minus the estimator's nuJ / J (nu_bar_planck_minus_estimator :342)
struct BinResidual {
  double nu_lower, nu_upper, nu_bar_estimator;
  AHD double operator()(const double T_R) const {
    return calculate_planck_mean_frequency(T_R, nu_lower, nu_upper) - nu_bar_estimator;
  }
};

// bits of one bin's outcome (counted per cell into ARTIS_RADFIELD_COUNT_*)
constexpr int BIN_AT_TRMIN = 1, BIN_AT_TRMAX = 2, BIN_RETRIED = 4, BIN_ZEROED = 8, BIN_NOTCONVERGED = 16;

// T_R of the bin: the TOMS 748 root in [500, 250000] K, or the bound beyond which the root lies
AHD float find_bin_T_R(const double nu_lower, const double nu_upper, const double nu_bar_estimator, int *bits, int *evals_out) {
  const BinResidual f{nu_lower, nu_upper, nu_bar_estimator};
  const double f_Tmin = f(BINS_T_R_MIN);
  const double f_Tmax = f(BINS_T_R_MAX);
  const bool invalid_values = (!isfinite(f_Tmin) || !isfinite(f_Tmax));
  *evals_out = 0;
  if (!invalid_values && f_Tmin * f_Tmax < 0) {
    int evals = MAXIT;
    const RootPair r = toms748(f, BINS_T_R_MIN, BINS_T_R_MAX, f_Tmin, f_Tmax, RelTol{1e-4}, &evals);
    *evals_out = evals;
    if (evals >= MAXIT) *bits |= BIN_NOTCONVERGED;
    return (float)(0.5 * (r.lo + r.hi));
  }
  if (invalid_values || f_Tmax < 0) return (float)BINS_T_R_MAX;
  return (float)BINS_T_R_MIN;
}

// (W, T_R) of bin b from its raw estimators, the cell's J_normfactor and T_e; returns the BIN_* bits
AHD int fit_bin(const double J_raw, const double nuJ_raw, const double J_normfactor, const int b, const float T_e, float *T_R_out,
                float *W_out) {
  const double nu_lower = bin_nu_lower(b);
  const double nu_upper = bin_nu_upper(b);
  const double J_bin = J_raw * J_normfactor;  // get_bin_J :185
  float T_R_bin = -1.;
  float W_bin = -1.;
  int bits = 0;
  if (J_bin > 0) {
    if (b == NBINS - 1) {
      T_R_bin = T_e;  // the T_e superbin
    } else {
      const double nuJ_bin = nuJ_raw * J_normfactor;  // get_bin_nuJ :193
      int evals = 0;
      T_R_bin = find_bin_T_R(nu_lower, nu_upper, nuJ_bin / J_bin, &bits, &evals);
      if (T_R_bin <= BINS_T_R_MIN) {
        bits |= BIN_AT_TRMIN;
      } else if (T_R_bin >= BINS_T_R_MAX) {
        bits |= BIN_AT_TRMAX;
      }
    }
    double planck_integral_result = calculate_planck_integral(T_R_bin, nu_lower, nu_upper, false);
    W_bin = (float)(J_bin / planck_integral_result);
    if (W_bin > 1e4 || !isfinite(W_bin)) {
      bits |= BIN_RETRIED;
      planck_integral_result = calculate_planck_integral(BINS_T_R_MAX, nu_lower, nu_upper, false);
      W_bin = (float)(J_bin / planck_integral_result);
      if (W_bin > 1e4) {
        bits |= BIN_ZEROED;
        T_R_bin = -99.;
        W_bin = 0.;
      } else {
        T_R_bin = BINS_T_R_MAX;
      }
    }
  } else {
    T_R_bin = 0.;
    W_bin = 0.;
  }
  *T_R_out = T_R_bin;
  *W_out = W_bin;
  return bits;
}

// ---- one cell (update_grid_cell update_grid.cc:462-573, set_params_fullspec radfield.cc:400, get_T_J_from_J :956)

struct CellIn {
  double J_raw, nuJ_raw;
  double assocvolume_tmin, prev_mid, tmin, deltat;
  int32_t nprocs, lte_iteration, thick;
  float TJ, TR, Te, W;  // the current cell state
};
struct CellOut {
  double J, nuJ, J_normfactor, estimator_normfactor;
  float TJ, TR, Te, W;
  int32_t flags;  // ARTIS_RADFIELD_* bits
};

AHD bool cell_is_fitted(const int32_t lte_iteration, const int32_t thick) { return !(lte_iteration || thick == ARTIS_CELL_THICK); }

// normalisation factors of one cell (the bound-free estimators use the first, J and the lines the second)
AHD void cell_normfactors(const double assocvolume_tmin, const double prev_mid, const double tmin, const double deltat,
                          const int32_t nprocs, double *estimator_normfactor, double *over4pi) {
  const double deltaV = assocvolume_tmin * rf_pow3(prev_mid / tmin);
  *estimator_normfactor = 1 / deltaV / deltat / nprocs;
  *over4pi = (1. / (4 * PI)) * *estimator_normfactor;
}

// clamp a temperature to [MINTEMP, MAXTEMP], setting the low / high flag
AHD float clamp_temperature(float T, const int32_t low_flag, const int32_t high_flag, int32_t *flags) {
  if (T > ARTIS_OPT_MAXTEMP) {
    *flags |= high_flag;
    T = ARTIS_OPT_MAXTEMP;
  } else if (T < ARTIS_OPT_MINTEMP) {
    *flags |= low_flag;
    T = ARTIS_OPT_MINTEMP;
  }
  return T;
}

AHD CellOut fit_cell(const CellIn &in) {
  CellOut o{};
  cell_normfactors(in.assocvolume_tmin, in.prev_mid, in.tmin, in.deltat, in.nprocs, &o.estimator_normfactor, &o.J_normfactor);
  o.J = in.J_raw * o.J_normfactor;  // normalise_J
  o.nuJ = in.nuJ_raw;
  o.TJ = in.TJ;
  o.TR = in.TR;
  o.Te = in.Te;
  o.W = in.W;
  o.flags = 0;
  if (!cell_is_fitted(in.lte_iteration, in.thick)) {
    float T_J = (float)pow(o.J * PI / STEBO, 1. / 4.);
    if (!isfinite(T_J)) {
      o.flags |= ARTIS_RADFIELD_TJ_KEPT;
      T_J = in.TJ;
    } else {
      T_J = clamp_temperature(T_J, ARTIS_RADFIELD_TJ_LOW, ARTIS_RADFIELD_TJ_HIGH, &o.flags);
    }
    o.TR = T_J;
    o.Te = T_J;
    o.TJ = T_J;
    o.W = 1;
    return o;
  }
  o.flags |= ARTIS_RADFIELD_FITTED;
  o.nuJ = in.nuJ_raw * o.J_normfactor;  // normalise_nuJ
  const double nubar = o.nuJ / o.J;
  if (!isfinite(nubar) || nubar == 0.) {
    o.flags |= ARTIS_RADFIELD_NUBAR_KEPT;
    return o;
  }
  o.TJ = clamp_temperature((float)pow(o.J * PI / STEBO, 1 / 4.), ARTIS_RADFIELD_TJ_LOW, ARTIS_RADFIELD_TJ_HIGH, &o.flags);
  o.TR = clamp_temperature((float)(H * nubar / KB / 3.832229494), ARTIS_RADFIELD_TR_LOW, ARTIS_RADFIELD_TR_HIGH, &o.flags);
  o.W = (float)(o.J * PI / STEBO / rf_pow4(o.TR));
  return o;
}

// normalise_bf_estimators radfield.cc:920
AHD float bfrate_normed(const double bfrate_raw, const double estimator_normfactor) {
  return (float)(bfrate_raw * (estimator_normfactor / H));
}
// normalise_J on a detailed line's estimator radfield.cc:893-899 (J_normfactor: cell_normfactors' over4pi)
AHD double Jb_lu_normed(const double Jb_lu_raw, const double J_normfactor) { return Jb_lu_raw * J_normfactor; }

// ---- one output element each: the bodies of the engine's kernels (stage_radfield.h) and of the loops of tests/radfield_host.
// Whoever calls them keeps one writer per element; the bin counts and the totals are summed by the caller.

// A cell that is not fitted keeps the bins of the cell state; its bound-free block is left as it is (prev_bfrate_normed of a
// THICK cell, and of every cell in an LTE iteration). Both follow from cell_is_fitted: update_grid_cell's one branch.
AHD bool cell_bins_carried_over(const int32_t lte_iteration, const int32_t thick) { return !cell_is_fitted(lte_iteration, thick); }
AHD bool cell_bf_rewritten(const int32_t lte_iteration, const int32_t thick) { return cell_is_fitted(lte_iteration, thick); }

// the per-cell outputs of the fit, [ncell] each; counts [ncell][ARTIS_RADFIELD_NCOUNTS]
struct CellArrays {
  double *J, *nuJ, *J_normfactor;
  float *TJ, *TR, *Te, *W;
  int32_t *flags, *counts;
};

// cell c: fit it, store its outputs, zero its bin counts
AHD void fit_cell_store(const int64_t c, const CellIn &in, const CellArrays &o) {
  const CellOut r = fit_cell(in);
  o.J[c] = r.J;
  o.nuJ[c] = r.nuJ;
  o.J_normfactor[c] = r.J_normfactor;
  o.TJ[c] = r.TJ;
  o.TR[c] = r.TR;
  o.Te[c] = r.Te;
  o.W[c] = r.W;
  o.flags[c] = r.flags;
  for (int k = 0; k < ARTIS_RADFIELD_NCOUNTS; k++) o.counts[c * ARTIS_RADFIELD_NCOUNTS + k] = 0;
}

// entry i = c * NBINS + b of a cell whose bins are carried over
AHD void carry_bin(const int64_t i, const float *prev_bin_T_R, const float *prev_bin_W, float *bin_T_R, float *bin_W) {
  bin_T_R[i] = prev_bin_T_R[i];
  bin_W[i] = prev_bin_W[i];
}
// entry i = c * nbf + k of a cell whose bound-free block is rewritten
AHD void bf_entry(const int64_t i, const double *bfrate_raw, const double estimator_normfactor, float *bf) {
  bf[i] = bfrate_normed(bfrate_raw[i], estimator_normfactor);
}
// entry i = c * nline + k of the detailed lines (the contribution count is passed on in the caller's types)
template <class CountIn, class CountOut>
AHD void line_entry(const int64_t i, const double *Jb_lu_raw, const CountIn *count_in, const double J_normfactor, double *Jb_lu,
                    CountOut *count_out) {
  Jb_lu[i] = Jb_lu_normed(Jb_lu_raw[i], J_normfactor);
  count_out[i] = count_in[i];
}

// entry i = c * NBINS + b of a fitted cell (flags, J_normfactor: fit_cell_store's; T_e: the cell state's): its (T_R, W) from the
// bin's raw estimators at *J_raw, *nuJ_raw. Returns the BIN_* bits, bit k being count k; 0 and nothing written in any other cell.
AHD int fit_bin_store(const int64_t i, const double *J_raw, const double *nuJ_raw, const int32_t *flags, const double *J_normfactor,
                      const float *T_e, float *bin_T_R, float *bin_W) {
  const int64_t c = i / NBINS;
  const int b = (int)(i - c * NBINS);
  if (!(flags[c] & ARTIS_RADFIELD_FITTED)) return 0;
  float T_R, W;
  const int bits = fit_bin(*J_raw, *nuJ_raw, J_normfactor[c], b, T_e[c], &T_R, &W);
  bin_T_R[i] = T_R;
  bin_W[i] = W;
  return bits;
}

}  // namespace artis_rf
