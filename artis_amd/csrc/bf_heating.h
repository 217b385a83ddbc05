// bf_heating.h -- the bound-free heating coefficients of one thin (fitted) cell: calculate_bfheatingcoeff / calculate_bfheatingcoeffs
// (thermalbalance.cc:194-252) and the bfheatingestimator renormalisation in front of them (update_grid.cc:412-443), with the adaptive
// 61-point Gauss-Kronrod integrator they use (gausskronrod.h: gauss_kronrod_integrate<61>(f, a, b, 15, 1e-3, &error)).
//
// The engine's kernels (stage_bfheat.h) and the loops of tests/bfheat_host (x86) call the same functions. Floating-point discipline as
// thermal_balance.h: -ffp-contract=off, every expression in the reference's order of operations; the integrand takes the thermal
// stage's own exp and expm1 (tb_exp, tb_expm1), so that a lane and the x86 build form the same bits.
//
// WHICH RADIATION FIELD. The ground integral of the renormalisation is taken before fit_parameters (update_grid.cc:569-575): it reads
// the RESIDENT T_R and W, as k_tb_renorm does for corrphotoionrenorm. The per-level integrals come after the fit and read the fit's.
//
// ONE NODE. The walk compares the unscaled Kronrod-Gauss difference with |scale x r1 x tol|, and scale = (b - a) / 2 is 1e14..1e16 Hz:
// on the step-function tables of the classic builds every integral ends after its first 61-point node. gk61_adaptive therefore
// evaluates the first node in registers and enters the generic depth-first walk (gk61_walk: not inlined, it holds the per-depth arrays)
// only when that node asks to subdivide.
#pragma once
#include "thermal_balance.h"

namespace artis_bfh {

using artis::DevModel;

// per-cell flag bits (include/artis_amd.h ARTIS_BFHEAT_*)
constexpr int32_t RENORM_ONE = 1, NONFINITE = 2;
constexpr int NTOTALS = 4;  // nodes evaluated, integrals that subdivided, integrals that reached depth 15, non-finite coefficients
constexpr unsigned MAX_DEPTH = 15;
constexpr double EPSREL = 1e-3;  // thermalbalance.cc:197
constexpr double FOURPI = 4 * artis::PI;

// ---------------------------------------------------------------- Gauss-Kronrod 61 (gausskronrod.h)
// Abscissae/weights of the 61-point Kronrod rule with its embedded 30-point Gauss rule: the QUADPACK dqk61 constants, stored as in
// gausskronrod.h:85-168 (zero first, then Gauss and Kronrod-only points interleaved in increasing order).
struct GK61 {
  double x[31];
  double w[31];
  double wg[15];
};
// (a function-local static constant: one copy in constant memory that a lane indexes in place; returned by value it would be
// rebuilt in every lane's scratch, since the rule's loops index it with a running i)
AHD const GK61 &gk61_tables() {
  static constexpr GK61 tables{
      {0.00000000000000000000000000000000000e+00, 5.14718425553176958330252131667225737e-02,
       1.02806937966737030147096751318000592e-01, 1.53869913608583546963794672743255920e-01,
       2.04525116682309891438957671002024710e-01, 2.54636926167889846439805129817805108e-01,
       3.04073202273625077372677107199256554e-01, 3.52704725530878113471037207089373861e-01,
       4.00401254830394392535476211542660634e-01, 4.47033769538089176780609900322854000e-01,
       4.92480467861778574993693061207708796e-01, 5.36624148142019899264169793311072794e-01,
       5.79345235826361691756024932172540496e-01, 6.20526182989242861140477556431189299e-01,
       6.60061064126626961370053668149270753e-01, 6.97850494793315796932292388026640068e-01,
       7.33790062453226804726171131369527646e-01, 7.67777432104826194917977340974503132e-01,
       7.99727835821839083013668942322683241e-01, 8.29565762382768397442898119732501916e-01,
       8.57205233546061098958658510658943857e-01, 8.82560535792052681543116462530225590e-01,
       9.05573307699907798546522558925958320e-01, 9.26200047429274325879324277080474004e-01,
       9.44374444748559979415831324037439122e-01, 9.60021864968307512216871025581797663e-01,
       9.73116322501126268374693868423706885e-01, 9.83668123279747209970032581605662802e-01,
       9.91630996870404594858628366109485725e-01, 9.96893484074649540271630050918695283e-01,
       9.99484410050490637571325895705810819e-01},
      {5.14947294294515675583404336470993075e-02, 5.14261285374590259338628792157812598e-02,
       5.12215478492587721706562826049442083e-02, 5.08817958987496064922974730498046919e-02,
       5.04059214027823468408930856535850289e-02, 4.97956834270742063578115693799423285e-02,
       4.90554345550297788875281653672381736e-02, 4.81858617570871291407794922983045926e-02,
       4.71855465692991539452614781810994865e-02, 4.60592382710069881162717355593735806e-02,
       4.48148001331626631923555516167232438e-02, 4.34525397013560693168317281170732581e-02,
       4.19698102151642461471475412859697578e-02, 4.03745389515359591119952797524681142e-02,
       3.86789456247275929503486515322810503e-02, 3.68823646518212292239110656171359677e-02,
       3.49793380280600241374996707314678751e-02, 3.29814470574837260318141910168539275e-02,
       3.09072575623877624728842529430922726e-02, 2.87540487650412928439787853543342111e-02,
       2.65099548823331016106017093350754144e-02, 2.41911620780806013656863707252320268e-02,
       2.18280358216091922971674857383389934e-02, 1.94141411939423811734089510501284559e-02,
       1.69208891890532726275722894203220924e-02, 1.43697295070458048124514324435800102e-02,
       1.18230152534963417422328988532505929e-02, 9.27327965951776342844114689202436042e-03,
       6.63070391593129217331982636975016813e-03, 3.89046112709988405126720184451550328e-03,
       1.38901369867700762455159122675969968e-03},
      {1.02852652893558840341285636705415044e-01, 1.01762389748405504596428952168554045e-01,
       9.95934205867952670627802821035694765e-02, 9.63687371746442596394686263518098651e-02,
       9.21225222377861287176327070876187672e-02, 8.68997872010829798023875307151257026e-02,
       8.07558952294202153546949384605297309e-02, 7.37559747377052062682438500221907342e-02,
       6.59742298821804951281285151159623612e-02, 5.74931562176190664817216894020561288e-02,
       4.84026728305940529029381404228075178e-02, 3.87991925696270495968019364463476920e-02,
       2.87847078833233693497191796112920436e-02, 1.84664683110909591423021319120472691e-02,
       7.96819249616660561546588347467362245e-03}};
  return tables;
}

// what a call of gk61_integrate did (the totals of a stage call are sums of these)
struct Gk61Stats {
  int32_t nodes;     // 61-point nodes evaluated
  int32_t maxdepth;  // the deepest node's depth (0: the first node sufficed)
};

// integrate_non_adaptive_m1_1<61> gausskronrod.h:173: the embedded Gauss rule has 30 points, so the centre is a Kronrod-only node
// (gauss_start = 1, kronrod_start = 2)
template <class F>
AHD double gk61_unit(const F &f, const GK61 &g, const double scale, const double mean, double *error) {
  const double fc = f((scale * 0.) + mean);
  double kr = fc * g.w[0];
  double gr = 0.;
  for (unsigned i = 1; i < 31; i += 2) {
    const double fp = f((scale * g.x[i]) + mean);
    const double fm = f((scale * -g.x[i]) + mean);
    kr += (fp + fm) * g.w[i];
    gr += (fp + fm) * g.wg[i / 2];
  }
  for (unsigned i = 2; i < 31; i += 2) {
    const double fp = f((scale * g.x[i]) + mean);
    const double fm = f((scale * -g.x[i]) + mean);
    kr += (fp + fm) * g.w[i];
  }
  *error = artis::dmax(fabs(kr - gr), fabs(kr * 2.220446049250313e-16 * 2));
  return kr;
}

// recursive_adaptive_integrate<61> gausskronrod.h:209 below a first node (a0, b0) that has asked to subdivide, as an explicit
// depth-first walk (gk31_adaptive's form, physics.h): node, left subtree, right subtree; estimate = left + right and the error
// accumulated as error_left += error_right at each split. abs_tol0: the first node's |estimate x tol|.
// Everything goes in and comes back by value, so that the caller keeps nothing addressable.
struct Gk61Walked {
  double estimate, error;
  int32_t nodes, maxdepth;  // of the walk alone (the first node is the caller's)
};
template <class F>
ANOINLINE Gk61Walked gk61_walk(const F f, const double tol, const double a0, const double b0, const double abs_tol0) {
  Gk61Walked out{0., 0., 0, 0};
  constexpr int MAXD = MAX_DEPTH + 1;
  // per depth: interval of the pending RIGHT child, its abs_tol, and the partial sums of the parent
  double ra[MAXD], rb[MAXD], rtol[MAXD], est_left[MAXD], err_left[MAXD];
  int state[MAXD];  // 0: left child in progress, 1: right child in progress
  const GK61 &g = gk61_tables();
  const double mid0 = (a0 + b0) / 2;
  ra[0] = mid0;
  rb[0] = b0;
  rtol[0] = abs_tol0 / 2;
  state[0] = 0;
  int depth = 1;
  double a = a0, b = mid0, abs_tol = abs_tol0 / 2;
  unsigned levels = MAX_DEPTH - 1;
  double ret_est = 0., ret_err = 0.;
  while (true) {
    double err_local = 0.;
    const double mean = (b + a) / 2;
    const double scale = (b - a) / 2;
    const double r1 = gk61_unit(f, g, scale, mean, &err_local);
    out.nodes++;
    if (depth > out.maxdepth) out.maxdepth = depth;
    const double estimate = scale * r1;
    const double abs_tol1 = fabs(estimate * tol);
    if (abs_tol == 0) abs_tol = abs_tol1;
    if ((levels != 0) && (abs_tol1 < err_local) && (abs_tol < err_local)) {
      const double mid = (a + b) / 2;
      ra[depth] = mid;
      rb[depth] = b;
      rtol[depth] = abs_tol / 2;
      state[depth] = 0;
      depth++;
      b = mid;
      abs_tol = abs_tol / 2;
      levels--;
      continue;
    }
    ret_est = estimate;
    ret_err = err_local;
    while (true) {  // unwind
      if (depth == 0) {
        out.estimate = ret_est;
        out.error = ret_err;
        return out;
      }
      const int d = depth - 1;
      if (state[d] == 0) {
        est_left[d] = ret_est;
        err_left[d] = ret_err;
        state[d] = 1;
        a = ra[d];
        b = rb[d];
        abs_tol = rtol[d];
        levels = MAX_DEPTH - depth;
        break;  // the right child
      }
      ret_est = est_left[d] + ret_est;
      ret_err = err_left[d] + ret_err;
      depth--;
    }
  }
}
// recursive_adaptive_integrate<61>(f, tol, a, b, 15, 0., error) for a < b: the first node here, the rest in gk61_walk
template <class F>
AHD double gk61_adaptive(const F &f, const double tol, const double a, const double b, double *error_out, Gk61Stats *st) {
  const GK61 &g = gk61_tables();
  double err_local = 0.;
  const double mean = (b + a) / 2;
  const double scale = (b - a) / 2;
  const double r1 = gk61_unit(f, g, scale, mean, &err_local);
  st->nodes = 1;
  st->maxdepth = 0;
  const double estimate = scale * r1;
  const double abs_tol1 = fabs(estimate * tol);  // abs_tol == 0 at the root: abs_tol = abs_tol1, and the two comparisons are one
  if (abs_tol1 < err_local) {
    const Gk61Walked w = gk61_walk(f, tol, a, b, abs_tol1);
    st->nodes += w.nodes;
    st->maxdepth = w.maxdepth;
    *error_out = w.error;
    return w.estimate;
  }
  *error_out = err_local;
  return estimate;
}
// gauss_kronrod_integrate<61>(f, a, b, 15, tol, error) gausskronrod.h:244 (finite bounds: the callers')
template <class F>
AHD double gk61_integrate(const F &f, const double a, const double b, const double tol, double *error_out, Gk61Stats *st) {
  st->nodes = 0;
  st->maxdepth = 0;
  if (a == b) return 0.;
  if (b < a) return -gk61_adaptive(f, tol, b, a, error_out, st);
  return gk61_adaptive(f, tol, a, b, error_out, st);
}

// the analytic integrands of tests/golden/gk61_reference.json, set (a): + - * / sqrt and comparisons only, so that the reference's
// integrator on x86, this one on x86 and this one on a lane see the same values (tests/golden/gk61_golden.cc holds them through this
// function; artis_amd_debug_gk61 runs them on the device)
struct Gk61TestFn {
  int32_t which;
  double p;
  int64_t *evals;
  AHD double operator()(const double x) const {
    ++*evals;
    switch (which) {
      case 0: return 1. + x * (p + x * x);                                  // a cubic
      case 1: return 1. / (1. + p * x * x);                                 // p = 1: 1 / (1 + x^2)
      case 2: return sqrt(x);                                               // (x >= 0)
      case 3: return fabs(x - p);                                           // p = 0.3: |x - 0.3|
      case 4: return (x < p) ? 1. : 2.;                                     // a step at p (irrational)
      case 5: { const double x2 = x * x, x4 = x2 * x2; return x4 * x4 * x2 - p * x4 * x + x; }  // degree 10
      case 6: return 1. / sqrt(x + p);                                      // an integrable singularity just outside
      default: return (x < p) ? 0. : sqrt(x - p);                           // a kink with an infinite slope at p
    }
  }
};

// ---------------------------------------------------------------- the integrand and one coefficient
// the exp and expm1 an integrand is formed with: the stage's own (tests/golden/gk61_golden.cc has libm's beside it)
struct TbMath {
  static AHD double exp(const double x) { return artis_tb::tb_exp(x); }
  static AHD double expm1(const double x) { return artis_tb::tb_expm1(x); }
};
// integrand_bfheatingcoeff thermalbalance.cc:38 with radfield() the dilute black body W x planck(nu, T_R) (radfield.cc:800,
// radfield.h:50)
template <class Math>
struct BfhIntegrand {
  int32_t npoints;  // the table's grid (DevModel NPHIXSPOINTS, NPHIXSNUINCREMENT, last_phixs_nuovernuedge), held by value
  double increment, last_nuovernuedge;
  const float *xs;
  double nu_edge;
  float T_R, W;
  AHD double operator()(const double nu) const {
    const float sigma_bf = artis::phixs_fromtable_grid(npoints, increment, last_nuovernuedge, xs, nu_edge, nu);
    const double planck = 2 * artis::HPLANCK * artis::pow3(nu) / artis::pow2(artis::CLIGHT) / Math::expm1(artis::HOVERKB * nu / T_R);
    return sigma_bf * (1 - (nu_edge / nu)) * (W * planck) * (1 - Math::exp(-artis::HOVERKB * nu / T_R));
  }
};
template <class Math>
AHD BfhIntegrand<Math> bfh_integrand(const DevModel &M, const float *xs, const double nu_edge, const float T_R, const float W) {
  return BfhIntegrand<Math>{(int32_t)M.NPHIXSPOINTS, M.NPHIXSNUINCREMENT, M.last_phixs_nuovernuedge, xs, nu_edge, T_R, W};
}

// the totals of one lane (or one x86 loop): integers, so that their sums do not depend on the order
struct Totals {
  int64_t v[NTOTALS];
  AHD void add(const Gk61Stats &s) {
    v[0] += s.nodes;
    v[1] += s.nodes > 1;
    v[2] += s.maxdepth >= (int32_t)MAX_DEPTH;
  }
};

// calculate_bfheatingcoeff thermalbalance.cc:194 of target t of level ul in the dilute black body (T_R, W)
AHD double bfh_coeff(const DevModel &M, const int ul, const int t, const float T_R, const float W, Totals *tot) {
  const int ui = M.level_ion[ul];
  const int element = M.ion_element[ui];
  const int ion = ui - M.elem_uniqueionindexstart[element];
  const int level = ul - M.ion_uniquelevelindexstart[ui];
  double error = 0.;
  const double E_threshold = artis::phixs_threshold(M, element, ion, level, t);
  const double nu_threshold = (1. / artis::HPLANCK) * E_threshold;
  const double nu_max_phixs = nu_threshold * M.last_phixs_nuovernuedge;
  const BfhIntegrand<TbMath> f = bfh_integrand<TbMath>(M, artis::phixs_table(M, ul), nu_threshold, T_R, W);
  Gk61Stats st;
  double bfheating = gk61_integrate(f, nu_threshold, nu_max_phixs, EPSREL, &error, &st);
  tot->add(st);
  bfheating *= FOURPI * artis::phixs_probability(M, ul, t);
  return bfheating;
}

// the renormalisation of one ground continuum (update_grid.cc:413-442): the estimator times estimator_normfactor over the analytic
// coefficient of the ground level's first target in the RESIDENT dilute black body. An integral that is not > 0 or a ratio that is
// not finite: 1, *fallback set.
AHD double bfh_ground_renorm(const DevModel &M, const int ul_ground, const double bfheatingestimator, const double estimator_normfactor,
                             const float T_R, const float W, int32_t *fallback, Totals *tot) {
  const double normed = bfheatingestimator * estimator_normfactor;
  const double bfheatingcoeff_ground = bfh_coeff(M, ul_ground, 0, T_R, W, tot);
  const double bfheatingrenorm = (bfheatingcoeff_ground > 0.) ? normed / bfheatingcoeff_ground : (double)INFINITY;
  if (isfinite(bfheatingrenorm)) return bfheatingrenorm;
  *fallback = 1;
  return 1.;
}

// calculate_bfheatingcoeffs thermalbalance.cc:229-248 of level ul: the targets in index order from 0., times the renormalisation of
// the level's closest ground continuum (renorm: the cell's row [nbfcontinua_ground]). elem_massfrac is read by builds without
// USE_ION_BFHEATING_ESTIMATORS only (the minelfrac rule).
AHD double bfh_level(const DevModel &M, const int ul, const float T_R, const float W, const double *renorm, const float elem_massfrac, Totals *tot) {
  const double minelfrac = 0.01;
  double bfheatingcoeff = 0.;
  if (elem_massfrac > minelfrac || ARTIS_OPT_USE_ION_BFHEATING_ESTIMATORS) {
    const int nphixstargets = M.level_nphixstargets[ul];
    for (int t = 0; t < nphixstargets; t++) bfheatingcoeff += bfh_coeff(M, ul, t, T_R, W, tot);
#if ARTIS_OPT_USE_ION_BFHEATING_ESTIMATORS
    const int ig = M.level_closestgroundlevelcont[ul];
    if (ig >= 0) bfheatingcoeff *= renorm[ig];
#endif
  }
  return bfheatingcoeff;
}

// ---- the arrays of all cells: what the kernels (device pointers) and the x86 loops (host pointers) hand to the bodies below
struct Arrays {
  int64_t ncell;
  int32_t nbfg;
  const float *res_TR, *res_W;  // the resident cell state: the ground integrals
  const float *lev_TR, *lev_W;  // the fit's (or the caller's): the levels' integrals
  const int32_t *fit_flags;
  const double *bfh_raw;  // bfheatingestimator[(c * nbfg + g) * bfh_stride]
  int32_t bfh_stride;
  const double *assocvol;
  double prev_mid, tmin, deltat;
  int32_t nprocs;
  const int32_t *gci;      // [nions] the ground continuum of every ion (-1: none)
  const float *massfrac;   // [ncell][nelements]; builds without USE_ION_BFHEATING_ESTIMATORS only
  const int32_t *levels;   // the levels that have targets, ascending
  int32_t nlevels_listed;
  double *renorm;  // [ncell][nbfg]
  double *coeffs;  // [ncell][nlevels]
  int32_t *flags;  // [ncell]
};
AHD bool cell_fitted(const Arrays &a, const int64_t c) { return (a.fit_flags[c] & ARTIS_RADFIELD_FITTED) != 0; }

// renorm[c][g]; returns the bits for the cell's flags. A cell that is not fitted, and a place no ion has: +0 (nothing reads it).
AHD int32_t ground_cell_entry(const DevModel &M, const Arrays &a, const int64_t c, const int g, Totals *tot) {
  const int64_t i = c * a.nbfg + g;
  const int ui = cell_fitted(a, c) ? artis_tb::ion_of_groundcont(M, a.gci, g) : -1;
  if (ui < 0) {
    a.renorm[i] = 0.;
    return 0;
  }
  double estimator_normfactor, over4pi;
  artis_rf::cell_normfactors(a.assocvol[c], a.prev_mid, a.tmin, a.deltat, a.nprocs, &estimator_normfactor, &over4pi);
  int32_t fallback = 0;
  const double r = bfh_ground_renorm(M, M.ion_uniquelevelindexstart[ui], a.bfh_raw[i * a.bfh_stride], estimator_normfactor, a.res_TR[c], a.res_W[c],
                                     &fallback, tot);
  a.renorm[i] = r;
  return fallback ? RENORM_ONE : 0;
}
// coeffs[c][levels[k]] of a fitted cell c (after the cell's ground entries); returns the bits for the cell's flags
AHD int32_t level_cell_entry(const DevModel &M, const Arrays &a, const int64_t c, const int k, Totals *tot) {
  const int ul = a.levels[k];
  const float massfrac = a.massfrac ? a.massfrac[c * M.nelements + M.ion_element[M.level_ion[ul]]] : 1.f;
  const double v = bfh_level(M, ul, a.lev_TR[c], a.lev_W[c], a.renorm + c * a.nbfg, massfrac, tot);
  a.coeffs[c * M.nlevels + ul] = v;
  if (isfinite(v)) return 0;
  tot->v[3] += 1;
  return NONFINITE;
}

}  // namespace artis_bfh
