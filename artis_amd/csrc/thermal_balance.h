// thermal_balance.h -- the thermal balance of one thin (fitted) cell: the photoionisation renormalisation and the Gamma per ground
// population in front of it (update_grid.cc:344-410, ratecoeff.cc:926-961), the heating and cooling rates at a trial T_e
// (thermalbalance.cc:78-188, kpkt.cc:57-302) and the T_e finder (call_T_e_finder thermalbalance.cc:258-333).
//
// The engine's kernels (stage_thermal.h) and the loops of tests/thermal_host (x86) call the same functions. Floating-point discipline as
// physics.h and ion_balance.h: -ffp-contract=off, every expression in the reference's order of operations and float/double mixing.
//
// Supported builds: ARTIS_TB_SUPPORTED below, the one condition. Three simplifications follow from it:
//   * LTEPOP_EXCITATION_USE_TJ == 1: partition functions and Boltzmann factors depend on T_J only, so they are fixed during the search
//     (U once per cell; e_l = exp(-E_l / KB / T_J) once per level and cell);
//   * the "> 10 % -> recompute Gamma" branch of T_e_eqn_heating_minus_cooling (thermalbalance.cc:131-148) is compiled out in the
//     reference too;
//   * NT_ON == 0: get_nt_frac_heating is 1 (nonthermal.cc).
//
// SUMMATION ORDER (this stage's contract; not the reference's sequential one). A rate is a sum over a flat list of the cell: the ions
// (free-free), the entries of alltrans in index order (collisional excitation: a downward entry is the term +0), the photoionisation
// targets in index order (collisional ionisation, free-bound, each +0 for a level that does not ionise) and the levels (bound-free
// heating). Lane l of 64 adds the terms l, l + 64, ... in order, starting from +0; combine64 adds the 64 partial sums in one fixed
// order. A wave does this with its lanes, the x86 build with a loop over the 64 "lanes". The rates of a trial state use the stage's own
// exp and log (tb_exp, tb_log below): given the same U and Gamma, the two machines form the same bits throughout the search. U
// (artis_ib::partfunct_entry) and Gamma (calculate_iongamma_per_gspop) keep libm's, as the ion balance has them.
#pragma once
#include "ion_balance.h"

#ifndef ARTIS_OPT_TEMPERATURE_SOLVER_ACCURACY
#error "include/artis_options.h defines ARTIS_OPT_TEMPERATURE_SOLVER_ACCURACY"
#endif

// the builds whose thermal balance these rules are (DIRECT_COL_HEAT == 0: heating_collisional is the estimator, thermalbalance.cc:115;
// no NLTE populations: what ARTIS_PRESET_NLTENEBULAR stands for in ion_balance.h's scope)
#if ARTIS_OPT_LTEPOP_EXCITATION_USE_TJ == 1 && ARTIS_OPT_USE_LUT_PHOTOION == 1 && ARTIS_OPT_NT_ON == 0 && ARTIS_OPT_DIRECT_COL_HEAT == 0 && \
    !defined(ARTIS_PRESET_NLTENEBULAR)
#define ARTIS_TB_SUPPORTED 1
#else
#define ARTIS_TB_SUPPORTED 0
#endif

namespace artis_tb {

using artis::DevModel;
using artis::KB;
using artis::eps;
using artis::ionstage;
using artis::lstart;
using artis::statw;
using artis::uion;
using artis_ib::MINPOP;

// the option that keeps this build from the stage (nullptr: supported)
inline const char *unsupported_option() {
  if (ARTIS_OPT_LTEPOP_EXCITATION_USE_TJ != 1) return "LTEPOP_EXCITATION_USE_TJ == 0";
  if (ARTIS_OPT_USE_LUT_PHOTOION != 1) return "USE_LUT_PHOTOION == 0";
  if (ARTIS_OPT_NT_ON != 0) return "NT_ON";
  if (ARTIS_OPT_DIRECT_COL_HEAT != 0) return "DIRECT_COL_HEAT";
  return ARTIS_TB_SUPPORTED ? nullptr : "NLTE populations";
}

constexpr double MINTEMP = ARTIS_OPT_MINTEMP, MAXTEMP = ARTIS_OPT_MAXTEMP;
constexpr double ACCURACY = ARTIS_OPT_TEMPERATURE_SOLVER_ACCURACY;
constexpr int TE_MAXIT = 100;  // thermalbalance.cc:281
constexpr int NLANES = 64;

// per-cell flag bits above the ion balance's (include/artis_amd.h ARTIS_THERMAL_*); the low byte: ARTIS_IONBAL_* of the last evaluation
constexpr int32_t BRACKETED = ARTIS_THERMAL_BRACKETED, PINNED_LOW = ARTIS_THERMAL_PINNED_LOW, PINNED_HIGH = ARTIS_THERMAL_PINNED_HIGH,
                  NONFINITE = ARTIS_THERMAL_NONFINITE, DAMPED_UP = ARTIS_THERMAL_DAMPED_UP, DAMPED_DOWN = ARTIS_THERMAL_DAMPED_DOWN,
                  MAXIT = ARTIS_THERMAL_MAXIT, RENORM_ONE = ARTIS_THERMAL_RENORM_ONE;

// the rates of one evaluation, in the order of artis_thermal_result.rates
constexpr int NRATES = ARTIS_THERMAL_NRATES;
enum Rate {
  COOLING_FF = 0,
  COOLING_COLLISIONAL,
  COOLING_FB,
  COOLING_ADIABATIC,
  HEATING_FF,
  HEATING_BF,
  HEATING_COLLISIONAL,
  HEATING_DEP,
  RESIDUAL,
  DEP_FRAC_HEATING
};

// ---- exp and log of the rates. A trial state's rates are formed with the stage's OWN exp and log, plain IEEE arithmetic in one fixed
// order (the rational forms of fdlibm's e_exp.c / e_log.c, below 1 ulp), so that a wave and the x86 build form the same bits: the
// search then takes the same path on both machines and every output is the same. (f64 +, -, x, / and sqrt are correctly rounded on
// both; -ffp-contract=off keeps the order.) Against libm's the values differ in a last bit, as two libms do.
// They exist for one reason: the stage's test contract holds a cell whose U and Gamma agree on both machines to bit-equal outputs,
// which two libms cannot give (measured with the device library's exp: Te_solved 2.3e-13 apart). tests/test_thermal_balance_rules.py
// holds tb_col_exc and tb_col_ion to physics.h's col_exc and col_ion over every transition and target, so the copies stay in step.
// The polynomial coefficients, the argument reductions and the forms of tb_exp and tb_log are those of fdlibm's e_exp.c and e_log.c:
/*
 * ====================================================
 * Copyright (C) 2004 by Sun Microsystems, Inc. All rights reserved. (e_exp.c)
 * Copyright (C) 1993 by Sun Microsystems, Inc. All rights reserved. (e_log.c)
 *
 * Developed at SunSoft, a Sun Microsystems, Inc. business.
 * Permission to use, copy, modify, and distribute this
 * software is freely granted, provided that this notice
 * is preserved.
 * ====================================================
 */
AHD double pow2i(const int k) {  // 2^k, -1022 <= k <= 1023
  union {
    uint64_t u;
    double d;
  } v;
  v.u = (uint64_t)(k + 1023) << 52;
  return v.d;
}
AHD double tb_exp(const double x) {
  if (x != x) return x;
  if (x > 709.782712893383973096) return (double)INFINITY;
  if (x < -745.13321910194110842) return 0.;
  const double ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10, invln2 = 1.44269504088896338700e+00;
  const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
               P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
  const int k = (int)(invln2 * x + ((x < 0) ? -0.5 : 0.5));
  const double t = k;
  const double hi = x - t * ln2HI;
  const double lo = t * ln2LO;
  const double r = hi - lo;
  const double z = r * r;
  const double c = r - z * (P1 + z * (P2 + z * (P3 + z * (P4 + z * P5))));
  const double y = 1. - ((lo - (r * c) / (2. - c)) - hi);
  if (k > 1023) return y * 2. * pow2i(k - 1);
  if (k < -1021) return y * pow2i(k + 1000) * pow2i(-1000);
  return y * pow2i(k);
}
AHD double tb_log(double x) {
  if (x != x) return x;
  if (x < 0.) return (double)NAN;
  if (x == 0.) return -(double)INFINITY;
  if (x > artis::DBLMAX) return x;
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
  const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
               Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
  int k = 0;
  if (x < 2.2250738585072014e-308) {  // subnormal: scale up
    x = x * 18014398509481984.;       // 2^54
    k = -54;
  }
  union {
    uint64_t u;
    double d;
  } v;
  v.d = x;
  uint32_t hx = (uint32_t)(v.u >> 32);
  k += (int)(hx >> 20) - 1023;
  hx &= 0x000fffffu;
  const uint32_t i = (hx + 0x95f64u) & 0x100000u;  // the mantissa into [sqrt(2)/2, sqrt(2))
  v.u = ((uint64_t)(hx | (i ^ 0x3ff00000u)) << 32) | (v.u & 0xffffffffull);
  k += (int)(i >> 20);
  const double f = v.d - 1.;
  const double s = f / (2. + f);
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double R = t2 + t1;
  const double hfsq = 0.5 * f * f;
  const double dk = k;
  return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}
// exp(x) - 1 for the bound-free heating integrand (bf_heating.h): the rational form and coefficients of fdlibm's s_expm1.c (same
// notice as above; Copyright (C) 1993 by Sun Microsystems, Inc.), the ranges chosen by comparing values, below 1 ulp
AHD double tb_expm1(double x) {
  if (x != x) return x;
  if (x > 709.782712893383973096) return (double)INFINITY;
  if (x < -38.816242111356935) return -1.;  // 56 ln2: exp(x) is below half an ulp of 1
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, invln2 = 1.44269504088896338700e+00;
  const double Q1 = -3.33333333333331316428e-02, Q2 = 1.58730158725481460165e-03, Q3 = -7.93650757867487942473e-05,
               Q4 = 4.00821782732936239552e-06, Q5 = -2.01099218183624371326e-07;
  const double ax = (x < 0) ? -x : x;
  int k = 0;
  double c = 0.;
  if (ax > 0.34657359027997264) {  // 0.5 ln2
    double hi, lo;
    if (ax < 1.0397207708399179) {  // 1.5 ln2
      if (x > 0) {
        hi = x - ln2_hi;
        lo = ln2_lo;
        k = 1;
      } else {
        hi = x + ln2_hi;
        lo = -ln2_lo;
        k = -1;
      }
    } else {
      k = (int)(invln2 * x + ((x < 0) ? -0.5 : 0.5));
      const double t = k;
      hi = x - t * ln2_hi;
      lo = t * ln2_lo;
    }
    x = hi - lo;
    c = (hi - x) - lo;
  } else if (ax < 5.551115123125783e-17) {  // 2^-54
    return x;
  }
  const double hfx = 0.5 * x;
  const double hxs = x * hfx;
  const double r1 = 1. + hxs * (Q1 + hxs * (Q2 + hxs * (Q3 + hxs * (Q4 + hxs * Q5))));
  double t = 3. - r1 * hfx;
  double e = hxs * ((r1 - t) / (6. - x * t));
  if (k == 0) return x - (x * e - hxs);
  e = (x * (e - c) - c);
  e = e - hxs;
  if (k == -1) return 0.5 * (x - e) - 0.5;
  if (k == 1) {
    if (x < -0.25) return -2. * (e - (x + 0.5));
    return 1. + 2. * (x - e);
  }
  if (k <= -2 || k > 56) {  // exp(x) - 1
    double y = 1. - (e - x);
    if (k == 1024)
      y = y * 2. * pow2i(1023);
    else
      y = y * pow2i(k);
    return y - 1.;
  }
  double y;
  if (k < 20) {
    t = 1. - pow2i(-k);
    y = t - (e - x);
    y = y * pow2i(k);
  } else {
    t = pow2i(-k);
    y = x - (e + t);
    y = y + 1.;
    y = y * pow2i(k);
  }
  return y;
}
// col_excitation_ratecoeff macroatom.cc:750 (physics.h col_exc) with the stage's exp and log
AHD double tb_col_exc(const DevModel &M, const float T_e, const float cnne, const double epsilon_trans, const double gu, const double gl, const int ati) {
  const float cs = M.alltrans_coll_str[ati];
  const double eoverkt = epsilon_trans / (KB * T_e);
  if (cs < 0) {
    if (!M.alltrans_forbidden[ati]) {
      const double f = M.alltrans_osc_strength[ati];
      const double g_bar = 0.2;
      const double ex = tb_exp(eoverkt);
      const double Gamma = artis::dmax(g_bar, 0.276 * ex * (-artis::EULERGAMMA - tb_log(eoverkt)));
      return artis::C_0 * cnne * sqrtf(T_e) * 14.51039491 * f * artis::pow2(artis::H_ionpot / epsilon_trans) * eoverkt / ex * Gamma;
    }
    return cnne * 8.629e-6 * 0.01 * tb_exp(-eoverkt) * gu / sqrtf(T_e);
  }
  return cnne * 8.629e-6 * (double)cs * tb_exp(-eoverkt) / gl / sqrtf(T_e);
}
// col_ionization_ratecoeff macroatom.cc:686 (physics.h col_ion) with the stage's exp; T_e^-0.5 as 1 / sqrt(T_e)
AHD double tb_col_ion(const DevModel &M, const float T_e, const float cnne, const int element, const int ion, const int lower, const int t,
                      const double epsilon_trans) {
  const int ul = lstart(M, element, ion) + lower;
  const double g = artis::gaunt_factor(ionstage(M, element, ion));
  const double fac1 = epsilon_trans / KB / T_e;
  const double sigma_bf = artis::phixs_table(M, ul)[0] * artis::phixs_probability(M, ul, t);
  return cnne * 1.55e13 * (1. / sqrt((double)T_e)) * g * sigma_bf * tb_exp(-fac1) / fac1;
}

// ---- the fixed order in which 64 partial sums become one: p[i] += p[i + h] for h = 32, 16, ... 1 (a wave forms the same sums with
// lane-xor exchanges of 32, 16, ... 1: lane 0's are these, addition commutes)
AHD double combine64(double *p) {
  for (int h = NLANES / 2; h >= 1; h >>= 1)
    for (int i = 0; i < h; i++) p[i] = p[i] + p[i + h];
  return p[0];
}
// the 64 "lanes" as a loop (x86; stage_thermal.h has the wave's form)
struct SeqLanes {
  template <class F>
  AHD double sum(const int n, F term) const {
    double p[NLANES];
    for (int l = 0; l < NLANES; l++) {
      double s = 0.;
      for (int i = l; i < n; i += NLANES) s += term(i);
      p[l] = s;
    }
    return combine64(p);
  }
  // every "lane" does entry(i) for its i (a wave: strided, then made visible to all lanes)
  template <class F>
  AHD void each(const int n, F entry) const {
    for (int i = 0; i < n; i++) entry(i);
  }
};

// ---- the renormalisation of one ground continuum (update_grid.cc:370-386): Gamma_normed over the analytic rate of the ground level's
// first target in the RESIDENT dilute black body (the reference renormalises before fit_parameters). A non-finite ratio or a
// non-positive denominator: 1, *fallback set.
AHD double renorm_entry(const DevModel &M, const int ul_ground, const double gamma_normed, const float W, const float T_R, int32_t *fallback) {
  const double gammacorr_ana = W * artis::lerp_or_last(M, M.corrphotoioncoeffs, ul_ground, 0, T_R);
  const double renorm = (gammacorr_ana > 0.) ? gamma_normed / gammacorr_ana : (double)INFINITY;
  if (isfinite(renorm)) return renorm;
  *fallback = 1;
  return 1.;
}
// the ion whose ground continuum is place g of the ground-continuum list (-1: none)
AHD int ion_of_groundcont(const DevModel &M, const int32_t *gci, const int g) {
  for (int ui = 0; ui < M.nions; ui++)
    if (gci[ui] == g) return ui;
  return -1;
}

// ---- calculate_levelpop ltepop.cc:412 / calculate_levelpop_boltzmann :395 from a ground population (physics.h populate_levelpop)
AHD double levelpop_lte(const DevModel &M, const int ul, const int start, const double nnground, const float massfrac, const float T_exc) {
  double nn;
  if (ul == start) {
    nn = nnground;
  } else {
    const double E_aboveground = eps(M, ul) - eps(M, start);
    nn = (nnground * statw(M, ul) / statw(M, start) * exp(-E_aboveground / KB / T_exc));
  }
  if (nn < MINPOP) nn = (massfrac > 0) ? MINPOP : 0.;
  return nn;
}
// the Boltzmann factor of a level, formed once per cell (T_exc = T_J)
AHD double boltzmann_e_l(const DevModel &M, const int ul, const float T_exc) {
  const double E_aboveground = eps(M, ul) - eps(M, M.ion_uniquelevelindexstart[M.level_ion[ul]]);
  return tb_exp(-E_aboveground / KB / T_exc);
}

// ---- calculate_iongamma_per_gspop ratecoeff.cc:926-961 of ion (element, ion) from the RESIDENT state (ground populations, T_J, W, T_R,
// T_e, n_e) with the cell's new renormalisation (get_corrphotoioncoeff ratecoeff.cc:858-866); sequential, in the reference's order
struct Resident {
  const float *ground;    // [nions]
  const float *massfrac;  // [nelements] (of the new timestep: the reference updates the composition first)
  float TJ, TR, W, Te, cnne;
};
AHD double iongamma_per_gspop(const DevModel &M, const int element, const int ion, const int32_t *gci, const Resident &r, const double *renorm) {
  const int nions = M.elem_nions[element];
  if (ion >= nions - 1) return 0.;
  const int ui = uion(M, element, ion);
  if (gci[ui] < 0) return 0.;
  const int start = lstart(M, element, ion), ustart = lstart(M, element, ion + 1);
  const int nlevels_ionising = M.ion_nlevels_ionising[ui];
  const double nnground = artis_ib::groundlevelpop(r.ground[ui], r.massfrac[element]);
  const double W = r.W;
  const double T_R = r.TR;
  double ionisation_rate_rad = 0.;
  double ionisation_rate_coll = 0.;
  for (int level = 0; level < nlevels_ionising; level++) {
    const int ul = start + level;
    const double nnlevel = levelpop_lte(M, ul, start, nnground, r.massfrac[element], r.TJ);
    const int nphixstargets = M.level_nphixstargets[ul];
    for (int t = 0; t < nphixstargets; t++) {
      const int upperlevel = artis::phixs_upperlevel(M, ul, t);
      double gammacorr = W * artis::lerp_or_last(M, M.corrphotoioncoeffs, ul, t, (float)T_R);
      const int ig = M.level_closestgroundlevelcont[ul];
      if (ig >= 0) gammacorr *= renorm[ig];
      ionisation_rate_rad += nnlevel * gammacorr;
      const double epsilon_trans = eps(M, ustart + upperlevel) - eps(M, ul);
      ionisation_rate_coll += nnlevel * artis::col_ion(M, r.Te, r.cnne, element, ion, level, t, epsilon_trans);
    }
  }
  const double ionisation_rate = (ionisation_rate_rad + ionisation_rate_coll);
  if (nnground <= 0.) return 0.;
  return ionisation_rate / nnground;
}

// ---- the state a rate is formed at: T_e, n_e, ground populations and partition functions; e_l [nlevels] the cell's Boltzmann factors
struct TrialState {
  float Te, cnne;
  const float *ground, *U;  // [nions]
  const float *massfrac;    // [nelements]
  const double *e_l;        // [nlevels]
};
AHD double nnion_at(const DevModel &M, const TrialState &s, const int ui) {  // get_nnion ltepop.h:106
  return artis_ib::groundlevelpop(s.ground[ui], s.massfrac[M.ion_element[ui]]) * s.U[ui] / statw(M, M.ion_uniquelevelindexstart[ui]);
}
// populate_levelpop's expression and order with the stored e_l; the MINPOP floor per evaluation
AHD double levelpop_at(const DevModel &M, const TrialState &s, const int ul) {
  const int ui = M.level_ion[ul];
  const int start = M.ion_uniquelevelindexstart[ui];
  const float massfrac = s.massfrac[M.ion_element[ui]];
  const double nnground = artis_ib::groundlevelpop(s.ground[ui], massfrac);
  double nn = (ul == start) ? nnground : (nnground * statw(M, ul) / statw(M, start) * s.e_l[ul]);
  if (nn < MINPOP) nn = (massfrac > 0) ? MINPOP : 0.;
  return nn;
}

// the terms of calculate_cooling_rates_ion<false> (kpkt.cc:57-229; physics.h cooling_ion_head, matrans_terms' kterm, cooling_ion_tail)
// free-free of ion ui (kpkt.cc:70-86)
AHD double cooling_ff_term(const DevModel &M, const TrialState &s, const int ui) {
  const int ioncharge = M.elem_lowest_ionstage[M.ion_element[ui]] + (ui - M.elem_uniqueionindexstart[M.ion_element[ui]]) - 1;
  if (ioncharge <= 0) return 0.;
  return 1.426e-27 * sqrt((double)s.Te) * artis::pow2(ioncharge) * nnion_at(M, s, ui) * s.cnne;
}
// collisional excitation of entry ati of alltrans (kpkt.cc:99-112): +0 for a downward entry
AHD double cooling_collexc_term(const DevModel &M, const TrialState &s, const int ati) {
  const int ul = M.alltrans_owner[ati];
  if (ati - M.level_alltrans_startdown[ul] < M.level_ndowntrans[ul]) return 0.;
  const int tul = M.ion_uniquelevelindexstart[M.level_ion[ul]] + M.alltrans_targetlevelindex[ati];
  const double epsilon_trans = eps(M, tul) - eps(M, ul);
  const double Cc = tb_col_exc(M, s.Te, s.cnne, epsilon_trans, statw(M, tul), statw(M, ul), ati);
  return levelpop_at(M, s, ul) * Cc * epsilon_trans;
}
// what a photoionisation target k (level ul, target t) belongs to; ionises: its level is an ionising level below the top ion
struct TargetOf {
  int ul, t, element, ion, level, ui;
  bool ionises;
};
AHD TargetOf target_of(const DevModel &M, const int32_t *target_level, const int k) {
  TargetOf r;
  r.ul = target_level[k];
  r.t = k - M.level_phixstargetstart[r.ul];
  r.ui = M.level_ion[r.ul];
  r.element = M.ion_element[r.ui];
  r.ion = r.ui - M.elem_uniqueionindexstart[r.element];
  r.level = r.ul - M.ion_uniquelevelindexstart[r.ui];
  r.ionises = r.ion < (M.elem_nions[r.element] - 1) && M.nbfcontinua > 0 && r.level < M.ion_nlevels_ionising[r.ui];
  return r;
}
// collisional ionisation through target k (kpkt.cc:130-158)
AHD double cooling_colion_term(const DevModel &M, const TrialState &s, const int32_t *target_level, const int k) {
  const TargetOf o = target_of(M, target_level, k);
  if (!o.ionises) return 0.;
  const double epsilon_trans = eps(M, M.ion_uniquelevelindexstart[o.ui + 1] + artis::phixs_upperlevel(M, o.ul, o.t)) - eps(M, o.ul);
  return levelpop_at(M, s, o.ul) * tb_col_ion(M, s.Te, s.cnne, o.element, o.ion, o.level, o.t, epsilon_trans) * epsilon_trans;
}
// free-bound through target k (kpkt.cc:161-220)
AHD double cooling_fb_term(const DevModel &M, const TrialState &s, const int32_t *target_level, const int k) {
  const TargetOf o = target_of(M, target_level, k);
  if (!o.ionises) return 0.;
  const int ustart = M.ion_uniquelevelindexstart[o.ui + 1];
  const int nt = M.level_nphixstargets[o.ul];
  double pop;
#if ARTIS_OPT_BFCOOLING_USELEVELPOPNOTIONPOP
  pop = levelpop_at(M, s, ustart + artis::phixs_upperlevel(M, o.ul, o.t));
#else
  const double nnupperion = nnion_at(M, s, o.ui + 1);
  if (nt == 1) {
    pop = nnupperion;
  } else {
    double E_min = artis::DBLMAX;
    for (int t = 0; t < nt; t++) E_min = artis::dmin(E_min, eps(M, ustart + artis::phixs_upperlevel(M, o.ul, t)));
    double wsum = 0.;
    for (int t = 0; t < nt; t++) {
      const int up = artis::phixs_upperlevel(M, o.ul, t);
      wsum += statw(M, ustart + up) * tb_exp(-(eps(M, ustart + up) - E_min) / KB / s.Te);
    }
    const int up = artis::phixs_upperlevel(M, o.ul, o.t);
    const double w = statw(M, ustart + up) * tb_exp(-(eps(M, ustart + up) - E_min) / KB / s.Te);
    pop = nnupperion * w / wsum;
  }
#endif
  return artis::lerp_or_last(M, M.bfcooling_coeffs, o.ul, o.t, s.Te) * pop * s.cnne;
}
// bound-free heating of level ul (thermalbalance.cc:96-104): +0 for a level that does not ionise
AHD double heating_bf_term(const DevModel &M, const TrialState &s, const double *bfheatingcoeffs, const int ul) {
  const int ui = M.level_ion[ul];
  const int element = M.ion_element[ui];
  if (ui - M.elem_uniqueionindexstart[element] >= M.elem_nions[element] - 1 || ul - M.ion_uniquelevelindexstart[ui] >= M.ion_nlevels_ionising[ui]) return 0.;
  return levelpop_at(M, s, ul) * bfheatingcoeffs[ul];
}

// heating_dep and dep_frac_heating (thermalbalance.cc:161-170) with get_nt_frac_heating == 1
AHD void heating_dep(const double ntlepton_dep, const double ntalpha_dep, const double ntspfission_dep, double *heating, double *frac) {
  const double ntlepton_frac_heating = 1.;
  *heating = (ntlepton_dep * ntlepton_frac_heating) + ntalpha_dep + ntspfission_dep;
  *frac = ((ntalpha_dep + ntspfission_dep) > 0) ? *heating / (ntlepton_dep + ntalpha_dep + ntspfission_dep) : ntlepton_frac_heating;
}
// adiabatic cooling (thermalbalance.cc:172-180)
AHD double cooling_adiabatic(const double nntot, const double T_e, const double volumetmin, const double tmin, const double t_current) {
  const double p = nntot * KB * T_e;
  const double dV_on_dt = 3 * volumetmin / artis::pow3(tmin) * artis::pow2(t_current);
  const double V = volumetmin * artis::pow3(t_current / tmin);
  return p * dV_on_dt / V;
}

// e_l of every level of a cell (the lanes share the levels; every lane sees all of them afterwards)
template <class Lanes>
AHD void fill_boltzmann(const DevModel &M, const float T_exc, double *e_l, const Lanes &lanes) {
  lanes.each(M.nlevels, [&](const int ul) { e_l[ul] = boltzmann_e_l(M, ul, T_exc); });
}

// ---- one cell of the solve: what is fixed during the search ...
struct CellFixed {
  float rho;
  const float *massfrac, *meanweight;  // [nelements] of the new timestep
  float clump, Te_old;
  const float *U;        // [nions] partition functions at the fit's T_J
  const double *gamma;   // [nbfcontinua_ground] Gamma per ground population (0 in a place no ion has)
  const double *e_l;     // [nlevels]
  const double *bfheatingcoeffs;  // [nlevels]
  const float *alpha_sp;
  const int32_t *gci, *target_level;
  int32_t nbfg;
  double heating_ff, heating_collisional;            // the estimators times estimator_normfactor (update_grid.cc:559-562)
  double ntlepton_dep, dep_alpha, dep_spfission;
  double assocvol, tmin, t_current;
};
// ... and what an evaluation leaves behind (the reference leaves the grid in the state of the last T_e, thermalbalance.cc:123-125)
struct CellWork {
  double *phi;         // [nions]
  float *ground;       // [nions]
  int32_t *uppermost;  // [nelements]
  float nne;
  int32_t ibflags;     // ARTIS_IONBAL_* of the last evaluation
  double rates[NRATES];
};

// the rates at T_e with the populations in w (T_e_eqn_heating_minus_cooling thermalbalance.cc:157-187)
template <class Lanes>
AHD double rates_at(const DevModel &M, const CellFixed &f, CellWork &w, const double T_e, const Lanes &lanes) {
  const auto fT_e = static_cast<float>(T_e);
  const TrialState s{fT_e, f.clump * w.nne, w.ground, f.U, f.massfrac, f.e_l};
  double *r = w.rates;
  r[COOLING_FF] = lanes.sum(M.nions, [&](const int ui) { return cooling_ff_term(M, s, ui); });
  const double C_exc = lanes.sum(M.nalltrans, [&](const int ati) { return cooling_collexc_term(M, s, ati); });
  const double C_ionisation = lanes.sum(M.nphixstargets_total, [&](const int k) { return cooling_colion_term(M, s, f.target_level, k); });
  r[COOLING_COLLISIONAL] = C_exc + C_ionisation;
  r[COOLING_FB] = lanes.sum(M.nphixstargets_total, [&](const int k) { return cooling_fb_term(M, s, f.target_level, k); });
  r[HEATING_BF] = lanes.sum(M.nlevels, [&](const int ul) { return heating_bf_term(M, s, f.bfheatingcoeffs, ul); });
  r[HEATING_FF] = f.heating_ff;
  r[HEATING_COLLISIONAL] = f.heating_collisional;
  heating_dep(f.ntlepton_dep, f.dep_alpha, f.dep_spfission, &r[HEATING_DEP], &r[DEP_FRAC_HEATING]);
  double nntot = 0.;  // get_nnion_tot atomic.h:51
  for (int element = 0; element < M.nelements; element++) nntot += artis_ib::elem_numberdens(f.massfrac[element], f.meanweight[element], f.rho);
  nntot = nntot + w.nne;
  r[COOLING_ADIABATIC] = cooling_adiabatic(nntot, T_e, f.assocvol, f.tmin, f.t_current);
  const double total_heating_rate = r[HEATING_FF] + r[HEATING_BF] + r[HEATING_COLLISIONAL] + r[HEATING_DEP];
  const double total_coolingrate = r[COOLING_FF] + r[COOLING_FB] + r[COOLING_COLLISIONAL] + r[COOLING_ADIABATIC];
  r[RESIDUAL] = total_heating_rate - total_coolingrate;
  return r[RESIDUAL];
}

// T_e_eqn_heating_minus_cooling thermalbalance.cc:126-188: the ion balance at T_e (phi of every ion with the rate-balance form and the
// new Gamma, then calculate_ion_balance_nne), then the rates. A balance that refuses the cell gives NaN.
template <class Lanes>
AHD double residual(const DevModel &M, const CellFixed &f, CellWork &w, const double T_e, const Lanes &lanes) {
  const auto fT_e = static_cast<float>(T_e);
  int32_t flags = 0;
  for (int ui = 0; ui < M.nions; ui++) artis_ib::phi_entry(M, 0, ui, flags, f.U, &fT_e, &f.clump, f.alpha_sp, f.gci, f.gamma, f.nbfg, w.phi);
  const artis_ib::Cell cell{f.rho, f.massfrac, f.meanweight, f.U, w.phi, f.gamma, f.gci, w.uppermost};
  float nne_root = 0.f;
  int evals = 0;
  w.nne = artis_ib::ion_balance_nne(M, cell, false, w.ground, &nne_root, &evals, &flags);
  w.ibflags = flags;
  if (flags & artis_ib::REFUSED) {
    for (int k = 0; k < NRATES; k++) w.rates[k] = (double)NAN;
    return w.rates[RESIDUAL];
  }
  return rates_at(M, f, w, T_e, lanes);
}

template <class Lanes>
struct Residual {
  const DevModel *M;
  const CellFixed *f;
  CellWork *w;
  const Lanes *lanes;
  AHD double operator()(const double T_e) const { return residual(*M, *f, *w, T_e, *lanes); }
};

// what the finder returns besides the state in CellWork
struct Found {
  float Te;          // the stored T_e
  double Te_solved;  // before the damping
  double a, b;       // the final bracket (a == b == Te_solved when there was none)
  int evals;         // evaluations of the residual, the two ends and the final one included
  int32_t flags;     // the thermal bits
};

// call_T_e_finder thermalbalance.cc:258-333
template <class Lanes>
AHD Found find_Te(const DevModel &M, const CellFixed &f, CellWork &w, const Lanes &lanes) {
  const Residual<Lanes> f_T_e{&M, &f, &w, &lanes};
  const double T_e_old = f.Te_old;
  Found out{};
  const double f_T_min = f_T_e(MINTEMP);
  const double f_T_max = f_T_e(MAXTEMP);
  out.evals = 2;
  const bool invalid_values = (!isfinite(f_T_min) || !isfinite(f_T_max));
  if (invalid_values) out.flags |= NONFINITE;
  double T_e;
  if (!invalid_values && f_T_min * f_T_max < 0) {
    int iternum = TE_MAXIT;
    const artis_rf::RootPair result = artis_rf::toms748(f_T_e, MINTEMP, MAXTEMP, f_T_min, f_T_max, artis_rf::RelTol{ACCURACY}, &iternum);
    out.evals += iternum;
    T_e = 0.5 * (result.lo + result.hi);
    out.a = result.lo;
    out.b = result.hi;
    out.flags |= BRACKETED;
    if (iternum >= TE_MAXIT) out.flags |= MAXIT;
  } else if (invalid_values || f_T_max < 0) {
    T_e = MINTEMP;
    out.a = out.b = T_e;
    out.flags |= PINNED_LOW;
  } else {
    T_e = MAXTEMP;
    out.a = out.b = T_e;
    out.flags |= PINNED_HIGH;
  }
  out.Te_solved = T_e;
  if (T_e > 2 * T_e_old) {
    T_e = artis::dmin(2 * T_e_old, MAXTEMP);
    out.flags |= DAMPED_UP;
  } else if (T_e < 0.5 * T_e_old) {
    T_e = artis::dmax(0.5 * T_e_old, MINTEMP);
    out.flags |= DAMPED_DOWN;
  }
  out.Te = static_cast<float>(T_e);
  // rates and populations of the final T_e (thermalbalance.cc:330-332), formed at the STORED float: what artis_amd_thermal_rates gives at
  // the same T_e (the reference passes the double on, which only its adiabatic term reads unrounded)
  f_T_e(static_cast<double>(out.Te));
  out.evals += 1;
  return out;
}

// ---- the arrays of all cells: what the kernels (device pointers) and the x86 loops (host pointers) hand to the bodies below
struct Arrays {
  int64_t ncell;
  int32_t nbfg;
  // the resident cell state (before the hand-over)
  const float *res_TJ, *res_TR, *res_W, *res_Te, *res_nne, *res_ground, *res_U;
  const double *res_renorm;
  // the last fit
  const float *fit_TJ;
  const int32_t *fit_flags;
  // the new timestep's matter and the clumping factors the balance uses
  const float *rho, *massfrac, *meanweight_cell, *meanweight_model, *clump;
  // estimators: gamma_raw[(c * nbfg + g) * gamma_stride], ff_raw / col_raw[c * est_stride]
  const double *gamma_raw, *ff_raw, *col_raw;
  int32_t gamma_stride, est_stride;
  const double *assocvol;
  double prev_mid, tmin, deltat;
  int32_t nprocs;
  // heating inputs
  const double *bfheatingcoeffs;  // [ncell][nlevels]
  const double *ntlepton_dep, *dep_alpha, *dep_spfission;
  // tables
  const float *alpha_sp;
  const int32_t *gci, *target_level;
  // outputs
  double *renorm, *gamma;  // [ncell][nbfg]
  float *U;                // [ncell][nions]
  float *Te, *nne;
  double *Te_solved, *bracket;  // [ncell], [ncell][2]
  int32_t *evals, *flags;
  double *rates;  // [ncell][NRATES]
  float *ground;  // [ncell][nions]
  double *phi;    // [ncell][nions]
};
AHD const float *cell_meanweight(const DevModel &M, const Arrays &a, const int64_t c) {
  return a.meanweight_cell ? a.meanweight_cell + c * M.nelements : a.meanweight_model;
}
AHD bool cell_fitted(const Arrays &a, const int64_t c) { return (a.fit_flags[c] & ARTIS_RADFIELD_FITTED) != 0; }

// the start of a call, one per cell: nothing solved (an unfitted cell stays so: T_e = the fit's, which is T_J there)
AHD void cell_clear(const DevModel &M, const Arrays &a, const int64_t c, const float *fit_Te) {
  a.Te[c] = fit_Te[c];
  a.Te_solved[c] = fit_Te[c];
  a.bracket[2 * c] = a.bracket[2 * c + 1] = fit_Te[c];
  a.evals[c] = 0;
  a.flags[c] = 0;
  a.nne[c] = a.res_nne[c];
  for (int k = 0; k < NRATES; k++) a.rates[c * NRATES + k] = 0.;
  for (int ui = 0; ui < M.nions; ui++) {
    a.ground[c * M.nions + ui] = a.res_ground[c * M.nions + ui];
    a.phi[c * M.nions + ui] = 0.;
  }
}
// renorm[c][g]; returns RENORM_ONE for the cell's flags where the fallback was taken. A cell that is not fitted, and a place no ion
// has, keep the resident value.
AHD int32_t renorm_cell_entry(const DevModel &M, const Arrays &a, const int64_t c, const int g) {
  const int64_t i = c * a.nbfg + g;
  const int ui = cell_fitted(a, c) ? ion_of_groundcont(M, a.gci, g) : -1;
  if (ui < 0) {
    a.renorm[i] = a.res_renorm[i];
    return 0;
  }
  const double gamma_normed = artis_ib::gamma_normed_entry(a.gamma_raw[i * a.gamma_stride], a.assocvol[c], a.prev_mid, a.tmin, a.deltat, a.nprocs);
  int32_t fallback = 0;
  a.renorm[i] = renorm_entry(M, M.ion_uniquelevelindexstart[ui], gamma_normed, a.res_W[c], a.res_TR[c], &fallback);
  return fallback ? RENORM_ONE : 0;
}
// gamma[c][gci[ui]] of ion ui (after the cell's renormalisation); an ion without a ground continuum writes nothing
AHD void gamma_cell_entry(const DevModel &M, const Arrays &a, const int64_t c, const int ui) {
  const int g = a.gci[ui];
  if (g < 0) return;
  double v = 0.;
  if (cell_fitted(a, c)) {
    const artis_ib::IonOf k = artis_ib::ion_of(M, ui);
    const Resident r{a.res_ground + c * M.nions, a.massfrac + c * M.nelements, a.res_TJ[c], a.res_TR[c], a.res_W[c], a.res_Te[c],
                     a.clump[c] * a.res_nne[c]};
    v = iongamma_per_gspop(M, k.element, k.ion, a.gci, r, a.renorm + c * a.nbfg);
  }
  a.gamma[c * a.nbfg + g] = v;
}

// what is fixed in cell c during its search; U, gamma, e_l: the cell's rows (the caller may have copied them closer)
AHD CellFixed cell_fixed(const DevModel &M, const Arrays &a, const int64_t c, const float *U, const double *gamma, const double *e_l) {
  CellFixed f{};
  f.rho = a.rho[c];
  f.massfrac = a.massfrac + c * M.nelements;
  f.meanweight = cell_meanweight(M, a, c);
  f.clump = a.clump[c];
  f.Te_old = a.res_Te[c];
  f.U = U;
  f.gamma = gamma;
  f.e_l = e_l;
  f.bfheatingcoeffs = a.bfheatingcoeffs + c * M.nlevels;
  f.alpha_sp = a.alpha_sp;
  f.gci = a.gci;
  f.target_level = a.target_level;
  f.nbfg = a.nbfg;
  double estimator_normfactor, over4pi;
  artis_rf::cell_normfactors(a.assocvol[c], a.prev_mid, a.tmin, a.deltat, a.nprocs, &estimator_normfactor, &over4pi);
  f.heating_ff = a.ff_raw[c * a.est_stride] * estimator_normfactor;
  f.heating_collisional = a.col_raw[c * a.est_stride] * estimator_normfactor;
  f.ntlepton_dep = a.ntlepton_dep[c];
  f.dep_alpha = a.dep_alpha[c];
  f.dep_spfission = a.dep_spfission[c];
  f.assocvol = a.assocvol[c];
  f.tmin = a.tmin;
  f.t_current = a.prev_mid;
  return f;
}
// artis_amd_thermal_rates: the rates of cell c at T_e. rebalance: the ion balance at T_e first (residual()); else with the n_e and
// the ground populations handed in through w (the resident ones), phi untouched
template <class Lanes>
AHD void rates_cell(const DevModel &M, const Arrays &a, const int64_t c, const CellFixed &f, CellWork &w, const float T_e, const bool rebalance,
                    const Lanes &lanes) {
  if (rebalance)
    residual(M, f, w, (double)T_e, lanes);
  else
    rates_at(M, f, w, (double)T_e, lanes);
}
// ... and its outputs (one writer: the caller picks the lane)
AHD void rates_store(const DevModel &M, const Arrays &a, const int64_t c, const float T_e, const bool rebalance, const CellWork &w) {
  a.Te[c] = T_e;
  a.nne[c] = w.nne;
  for (int k = 0; k < NRATES; k++) a.rates[c * NRATES + k] = w.rates[k];
  for (int ui = 0; ui < M.nions; ui++) {
    a.ground[c * M.nions + ui] = w.ground[ui];
    a.phi[c * M.nions + ui] = rebalance ? w.phi[ui] : 0.;
  }
  if (rebalance) a.flags[c] = (a.flags[c] & ~0xFF) | (w.ibflags & 0xFF);
}

// the outputs of cell c from the finder's result and the state it left (one writer: the caller picks the lane)
AHD void cell_store(const DevModel &M, const Arrays &a, const int64_t c, const Found &r, const CellWork &w) {
  a.Te[c] = r.Te;
  a.Te_solved[c] = r.Te_solved;
  a.bracket[2 * c] = r.a;
  a.bracket[2 * c + 1] = r.b;
  a.evals[c] = r.evals;
  a.flags[c] = a.flags[c] | r.flags | (w.ibflags & 0xFF);
  a.nne[c] = w.nne;
  for (int k = 0; k < NRATES; k++) a.rates[c * NRATES + k] = w.rates[k];
  for (int ui = 0; ui < M.nions; ui++) {
    a.ground[c * M.nions + ui] = w.ground[ui];
    a.phi[c * M.nions + ui] = w.phi[ui];
  }
}

}  // namespace artis_tb
