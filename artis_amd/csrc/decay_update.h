// decay_update.h -- the decay and abundance update of the grid update, per decay path, per nuclide, per (cell, nuclide) and per
// (cell, element).
//
// What the reference does to every cell's composition at the start of update_grid (update_grid.cc:710-720): the Bateman sum of every
// decay path at t_mid - t_model (calculate_decaychain decay.h:56, without the expansion factor), from it one coefficient per path
// for the path's end nuclide and one for He4 (calc_nuc_massfrac_coeffs decay.cc:1284), every nuclide's surviving fraction; per cell
// the nuclides' mass fractions as the sparse product of those coefficients with the initial mass fractions (calc_cell_nuc_massfracs
// decay.cc:1204), the elements' mass fractions and mean weights (update_abundances decay.cc:1230) and the density (update_grid.cc:718).
// The engine's kernels (stage_decay.h) and the loops of tests/decay_host (x86) call the same bodies.
//
// The product's static structure -- which paths feed which nuclide, in path order -- is built once on the host (build_rows). A row
// entry names its coefficient by one index into the array [2 * npaths] {endnuc_coeff[npaths], he4_coeff[npaths]}.
//
// Floating-point discipline as physics.h: -ffp-contract=off, and every expression keeps the reference's order of operations.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "physics.h"

namespace artis_decay {

constexpr double DBL_EPS = 2.220446049250313080847e-16;
constexpr double DBL_MINV = 2.2250738585072014e-308;

// ---- the Bateman sum

struct Chain {
  double abund;  // the chain-end abundance per unit initial abundance of the top (clamped to 0 where the sum has no significance)
  double scale;  // lambdaproduct * the largest |term|: what the sum's rounding is measured in
  double x_dom;  // lambda_j * timediff of that largest term
};

// lambdas[0 .. n): 1 / mean life along the path; zero_last: the last one counts as 0 (the end taken as stable).
// The clamps are the reference's (a negative sum, or one below n eps x its largest term, has no significance), and one more: a sum
// whose scale has underflowed (below DBL_MIN: every exp has left the normal range, the terms carry no relative precision) is 0 too,
// where the reference returns a subnormal number of no meaning (below 1e-307 per unit initial abundance).
AHD Chain decaychain(const double *lambdas, const int n, const double timediff, const bool zero_last) {
  const auto lam = [&](int i) { return (zero_last && i == n - 1) ? 0. : lambdas[i]; };
  double lambdaproduct = 1.;
  for (int j = 0; j < n - 1; j++) lambdaproduct *= lam(j);
  double sum = 0., maxabsterm = 0., x_dom = 0.;
  for (int j = 0; j < n; j++) {
    const double lambda_j = lam(j);
    double denominator = 1.;
    for (int p = 0; p < n; p++)
      if (p != j) denominator *= (lam(p) - lambda_j);
    const double term = exp(-lambda_j * timediff) / denominator;
    sum += term;
    const double absterm = fabs(term);
    if (absterm > maxabsterm) {
      maxabsterm = absterm;
      x_dom = lambda_j * timediff;
    }
  }
  const double last = lambdaproduct * sum;
  Chain r{last, lambdaproduct * maxabsterm, x_dom};
  if (last < 0. || fabs(sum) <= n * DBL_EPS * maxabsterm || r.scale < DBL_MINV) r.abund = 0.;
  return r;
}
AHD Chain decaychain(const double *lambdas, const int n, const double timediff) { return decaychain(lambdas, n, timediff, false); }

// ---- tables: a view of host or device arrays

struct Tables {
  int32_t nnuclides, npaths, nelements, he4_nucindex;
  // per nuclide
  const double *nuc_lambda;  // meanlife > 0 ? 1 / meanlife : 0
  const double *nuc_mass;    // A * MH
  // per path: its nuclides [path_start[p], path_start[p + 1]) top ... end, and their lambdas beside them
  const int32_t *path_start, *path_nucindex;
  const double *path_lambda, *path_branchproduct;
  const int32_t *path_last_decaytype;
  // rows: nuclide n takes the entries [row_start[n], row_start[n + 1]), in path order; row_coef indexes {endnuc_coeff, he4_coeff}
  const int32_t *row_start, *row_coef, *row_top;
  // element e holds the nuclides elem_nuc[elem_nuc_start[e] .. elem_nuc_start[e + 1]), in nuclide order
  const int32_t *elem_nuc_start, *elem_nuc;
  const float *elem_initstablemeannucmass;
};

// the coefficients a timestep's update works with: coef [2 * npaths] {endnuc_coeff, he4_coeff}, survivingfrac [nnuclides]
struct Coeffs {
  const double *coef, *survivingfrac;
};

// one path's two coefficients (decay.cc:1295-1310) and the end chain's scale and x_dom
AHD void path_coeffs(const Tables &T, const int p, const double t_afterinit, double *endnuc_coeff, double *he4_coeff, double *scale,
                     double *x_dom) {
  const int i0 = T.path_start[p], n = T.path_start[p + 1] - i0;
  const int top = T.path_nucindex[i0], end = T.path_nucindex[i0 + n - 1];
  const Chain ch = decaychain(T.path_lambda + i0, n, t_afterinit, false);
  endnuc_coeff[p] = T.path_branchproduct[p] * ch.abund * T.nuc_mass[end] / T.nuc_mass[top];
  scale[p] = ch.scale;
  x_dom[p] = ch.x_dom;
  double he4 = 0.;
  if (T.he4_nucindex >= 0 && T.path_last_decaytype[p] == ARTIS_DECAYTYPE_ALPHA && end != T.he4_nucindex)
    he4 = T.path_branchproduct[p] * decaychain(T.path_lambda + i0, n, t_afterinit, true).abund * T.nuc_mass[T.he4_nucindex] / T.nuc_mass[top];
  he4_coeff[p] = he4;
}

AHD double nuc_survivingfrac(const Tables &T, const int nuc, const double t_afterinit) { return exp(-t_afterinit * T.nuc_lambda[nuc]); }

// ---- per cell. X is [nuclide][cell] (stride cells per nuclide), float

// the mass fraction of one nuclide in one cell: its surviving initial share, then its row's additions in path order. The loads of
// four entries are issued before their dependent additions.
AHD double nuc_massfrac(const Tables &T, const Coeffs &K, const float *X, const int64_t stride, const int64_t c, const int nuc) {
  double mf = K.survivingfrac[nuc] * (double)X[(int64_t)nuc * stride + c];
  int k = T.row_start[nuc];
  const int k1 = T.row_start[nuc + 1];
  for (; k + 4 <= k1; k += 4) {
    const float x0 = X[(int64_t)T.row_top[k] * stride + c], x1 = X[(int64_t)T.row_top[k + 1] * stride + c];
    const float x2 = X[(int64_t)T.row_top[k + 2] * stride + c], x3 = X[(int64_t)T.row_top[k + 3] * stride + c];
    mf += K.coef[T.row_coef[k]] * (double)x0;
    mf += K.coef[T.row_coef[k + 1]] * (double)x1;
    mf += K.coef[T.row_coef[k + 2]] * (double)x2;
    mf += K.coef[T.row_coef[k + 3]] * (double)x3;
  }
  for (; k < k1; k++) mf += K.coef[T.row_coef[k]] * (double)X[(int64_t)T.row_top[k] * stride + c];
  return mf;
}

// one element of one cell (decay.cc:1249-1276): untracked is [cell][element]
AHD void element_entry(const Tables &T, const Coeffs &K, const float *X, const int64_t stride, const int64_t c, const int el,
                       const float *untracked, float *elem_massfracs, float *elem_meanweight) {
  double sum = 0., sum_on_mass = 0.;
  for (int i = T.elem_nuc_start[el]; i < T.elem_nuc_start[el + 1]; i++) {
    const int nuc = T.elem_nuc[i];
    const double mf = nuc_massfrac(T, K, X, stride, c, nuc);
    sum += mf;
    sum_on_mass += mf / T.nuc_mass[nuc];
  }
  const double otherstable = untracked[c * T.nelements + el];
  const double isosum = sum + otherstable;
  const double isosum_on_mass = sum_on_mass + (otherstable / T.elem_initstablemeannucmass[el]);
  elem_massfracs[c * T.nelements + el] = (float)isosum;
  const float meanweight = (float)(isosum / isosum_on_mass);
  elem_meanweight[c * T.nelements + el] = (isfinite(meanweight) && meanweight > 0.) ? meanweight : T.elem_initstablemeannucmass[el];
}

// update_grid.cc:691, :718
AHD float cell_rho(const float rho_tmin, const double t_mid, const double tmin) {
  const double r = t_mid / tmin;
  return (float)(rho_tmin / (r * r * r));
}

// ---- host: validation and the row structure (plain C++)

struct Rows {
  std::vector<double> nuc_lambda, nuc_mass, path_lambda;
  std::vector<int32_t> row_start, row_coef, row_top, row_path, row_kind;  // (path, kind: 0 end, 1 He4) beside the packed index
  std::vector<int32_t> elem_nuc_start, elem_nuc, nuc_element;
  int32_t he4_nucindex = -1;
};

// empty: the model is usable; else what is wrong with it, naming the path. ncell, nelements: the sizes of the per-cell arrays, which
// are checked when ncell > 0
inline std::string decay_validate(const artis_decay_model &d, const int64_t ncell = 0, const int nelements = 0) {
  const auto finite_nonneg = [](double v) { return std::isfinite(v) && v >= 0.; };
  if (d.nnuclides < 0 || d.npaths < 0) return "a negative count";
  if (d.nnuclides > 0 && (!d.nuc_z || !d.nuc_a || !d.nuc_meanlife)) return "nuc_z, nuc_a and nuc_meanlife are required";
  if (d.npaths > 0 && (!d.path_start || !d.path_nucindex || !d.path_branchproduct || !d.path_last_decaytype))
    return "path_start, path_nucindex, path_branchproduct and path_last_decaytype are required";
  if (!std::isfinite(d.t_model) || d.t_model < 0.) return "t_model is non-finite or negative";
  for (int n = 0; n < d.nnuclides; n++) {
    if (!std::isfinite(d.nuc_meanlife[n])) return "nuclide " + std::to_string(n) + ": a non-finite mean life";
    if (d.nuc_a[n] <= 0 || d.nuc_z[n] < 0) return "nuclide " + std::to_string(n) + ": Z < 0 or A <= 0";
  }
  if (d.npaths > 0 && d.path_start[0] != 0) return "path_start[0] is not 0";
  for (int p = 0; p < d.npaths; p++) {
    const std::string name = "path " + std::to_string(p) + ": ";
    const int64_t i0 = d.path_start[p], len = (int64_t)d.path_start[p + 1] - i0;
    if (len < 2) return name + "shorter than 2 nuclides";
    if (!finite_nonneg(d.path_branchproduct[p])) return name + "a non-finite or negative branchproduct";
    for (int64_t i = 0; i < len; i++) {
      const int nuc = d.path_nucindex[i0 + i];
      if (nuc < 0 || nuc >= d.nnuclides) return name + "a nuclide index out of range";
      if (i < len - 1 && !(d.nuc_meanlife[nuc] > 0.)) return name + "a nuclide before the end with meanlife <= 0";
    }
    for (int64_t i = 0; i < len; i++)
      for (int64_t j = i + 1; j < len; j++) {
        const double mi = d.nuc_meanlife[d.path_nucindex[i0 + i]], mj = d.nuc_meanlife[d.path_nucindex[i0 + j]];
        if (mi > 0. && mj > 0. && 1. / mi == 1. / mj) return name + "two nuclides with equal decay constants (the Bateman sum is singular)";
      }
  }
  if (ncell > 0) {
    if (!d.initnucmassfrac || !d.elem_untrackedstable_initmassfrac || !d.elem_initstablemeannucmass || !d.rho_tmin)
      return "initnucmassfrac, elem_untrackedstable_initmassfrac, elem_initstablemeannucmass and rho_tmin are required";
    const auto bad = [&](const float *a, int64_t n) {
      for (int64_t i = 0; i < n; i++)
        if (!finite_nonneg(a[i])) return true;
      return false;
    };
    if (bad(d.initnucmassfrac, ncell * d.nnuclides)) return "initnucmassfrac: a non-finite or negative entry";
    if (bad(d.elem_untrackedstable_initmassfrac, ncell * nelements)) return "elem_untrackedstable_initmassfrac: a non-finite or negative entry";
    if (bad(d.elem_initstablemeannucmass, nelements)) return "elem_initstablemeannucmass: a non-finite or negative entry";
    if (bad(d.rho_tmin, ncell)) return "rho_tmin: a non-finite or negative entry";
  }
  return "";
}

// of a validated model. elem_anumber [nelements]: the model's elements
inline Rows build_rows(const artis_decay_model &d, const int32_t *elem_anumber, const int nelements) {
  Rows r;
  const int nn = d.nnuclides;
  r.nuc_lambda.resize((size_t)nn);
  r.nuc_mass.resize((size_t)nn);
  r.nuc_element.assign((size_t)nn, -1);
  for (int n = 0; n < nn; n++) {
    r.nuc_lambda[(size_t)n] = d.nuc_meanlife[n] > 0. ? 1. / d.nuc_meanlife[n] : 0.;
    r.nuc_mass[(size_t)n] = d.nuc_a[n] * artis::MH;
    if (d.nuc_z[n] == 2 && d.nuc_a[n] == 4 && r.he4_nucindex < 0) r.he4_nucindex = n;
    for (int el = 0; el < nelements; el++)
      if (elem_anumber[el] == d.nuc_z[n]) {
        r.nuc_element[(size_t)n] = el;
        break;
      }
  }
  const int64_t nflat = d.npaths > 0 ? d.path_start[d.npaths] : 0;
  r.path_lambda.resize((size_t)nflat);
  for (int64_t i = 0; i < nflat; i++) r.path_lambda[(size_t)i] = r.nuc_lambda[(size_t)d.path_nucindex[i]];
  // rows: count, then fill in path order (for He4 a path's end entry comes before its He4 entry)
  std::vector<std::vector<int32_t>> rows((size_t)nn);  // packed: 2 * path + kind
  for (int p = 0; p < d.npaths; p++) {
    const int end = d.path_nucindex[d.path_start[p + 1] - 1];
    rows[(size_t)end].push_back(2 * p);
    if (r.he4_nucindex >= 0 && d.path_last_decaytype[p] == ARTIS_DECAYTYPE_ALPHA && end != r.he4_nucindex)
      rows[(size_t)r.he4_nucindex].push_back(2 * p + 1);
  }
  r.row_start.assign((size_t)nn + 1, 0);
  for (int n = 0; n < nn; n++) {
    r.row_start[(size_t)n + 1] = r.row_start[(size_t)n] + (int32_t)rows[(size_t)n].size();
    for (int32_t e : rows[(size_t)n]) {
      const int p = e / 2, kind = e % 2;
      r.row_path.push_back(p);
      r.row_kind.push_back(kind);
      r.row_coef.push_back(kind ? d.npaths + p : p);
      r.row_top.push_back(d.path_nucindex[d.path_start[p]]);
    }
  }
  r.elem_nuc_start.assign((size_t)nelements + 1, 0);
  for (int el = 0; el < nelements; el++) {
    for (int n = 0; n < nn; n++)
      if (r.nuc_element[(size_t)n] == el) r.elem_nuc.push_back(n);
    r.elem_nuc_start[(size_t)el + 1] = (int32_t)r.elem_nuc.size();
  }
  return r;
}

// the view of a model's host arrays and its rows
inline Tables host_tables(const artis_decay_model &d, const Rows &r, const int nelements) {
  Tables T{};
  T.nnuclides = d.nnuclides;
  T.npaths = d.npaths;
  T.nelements = nelements;
  T.he4_nucindex = r.he4_nucindex;
  T.nuc_lambda = r.nuc_lambda.data();
  T.nuc_mass = r.nuc_mass.data();
  T.path_start = d.path_start;
  T.path_nucindex = d.path_nucindex;
  T.path_lambda = r.path_lambda.data();
  T.path_branchproduct = d.path_branchproduct;
  T.path_last_decaytype = d.path_last_decaytype;
  T.row_start = r.row_start.data();
  T.row_coef = r.row_coef.data();
  T.row_top = r.row_top.data();
  T.elem_nuc_start = r.elem_nuc_start.data();
  T.elem_nuc = r.elem_nuc.data();
  T.elem_initstablemeannucmass = d.elem_initstablemeannucmass;
  return T;
}

}  // namespace artis_decay
