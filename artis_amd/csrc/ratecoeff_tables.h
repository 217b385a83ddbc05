// ratecoeff_tables.h -- the temperature tables of the rate coefficients: precalculate_rate_coefficient_integrals (ratecoeff.cc:143-233)
// with its three integrands (ratecoeff.cc:75-121) on the adaptive 61-point Gauss-Kronrod integrator of bf_heating.h
// (integrator<61>: gauss_kronrod_integrate<61>(f, a, b, 15, RATECOEFF_INTEGRAL_ACCURACY, &error), integrator.h:61).
//
// The engine's kernel (stage_ratecoeff.h) and the loops of tests/ratecoeff_host (x86) call the same functions. Floating-point discipline
// as bf_heating.h: -ffp-contract=off, every expression in the reference's order of operations and float/double mixing. The integrands
// are templated on a Math policy: the stage's own exp and expm1 (artis_bfh::TbMath: a lane and the x86 build form the same bits) or
// libm's (the reference's arithmetic; the x86 harness builds both).
//
// TWO FORMS. rc_entry is the reference's: one gk61_integrate call per table and entry. rc_entry_shared forms the entry's alpha_sp and
// bfcooling integrals from ONE set of evaluations: both run over nu - nu_edge on [0, nu_max_phixs - nu_threshold], so the first node's
// 61 abscissae, the cross-section there and exp(-HOVERKB x / T_e) are the same expressions in both; each sum is then taken in the
// rule's order (Gauss loop, Kronrod loop). An integral whose first node asks to subdivide is handed to gk61_integrate as it is, so the
// general walk is kept. gammacorr has its own interval ([nu_threshold, nu_max_phixs]: scale x + mean differs in the last bit) and shares
// nothing. The two forms give the same bits (tests/test_ratecoeff_rules.py holds every entry to that).
//
// Tpow[t] = std::pow((float)T, -1.5) is made on the HOST with the host's libm (make_tpow) and handed in as TABLESIZE doubles: the
// device's pow does not enter.
#pragma once
#include <vector>

#include "bf_heating.h"

namespace artis_rc {

using artis::DevModel;
using artis_bfh::GK61;
using artis_bfh::Gk61Stats;
using artis_bfh::TbMath;

constexpr int TABLESIZE = ARTIS_OPT_TABLESIZE;
constexpr double EPSREL = 1e-3;  // RATECOEFF_INTEGRAL_ACCURACY ratecoeff.cc:37
constexpr double FOURPI = 4 * artis::PI;
// the tables of an entry, in the order the reference fills them (gammacorr: builds with USE_LUT_PHOTOION only)
constexpr int KIND_ALPHA_SP = 0, KIND_GAMMACORR = 1, KIND_BFCOOLING = 2;
// per-entry flag bits (include/artis_amd.h ARTIS_RATECOEFF_*): what the reference would assert_always on
constexpr int32_t BAD_ALPHA_SP = ARTIS_RATECOEFF_BAD_ALPHA_SP, BAD_GAMMACORR = ARTIS_RATECOEFF_BAD_GAMMACORR,
                  BAD_BFCOOLING = ARTIS_RATECOEFF_BAD_BFCOOLING, BAD_SAHAFACT = ARTIS_RATECOEFF_BAD_SAHAFACT;
constexpr int NTOTALS = 4;  // integrals, 61-point nodes evaluated, integrals that reached depth 15, flagged entries

// the totals of one lane (or one x86 loop): integers, so that their sums do not depend on the order
struct Totals {
  int64_t v[NTOTALS];
  AHD void add(const Gk61Stats &s) {
    v[0] += 1;
    v[1] += s.nodes;
    v[2] += s.maxdepth >= (int32_t)artis_bfh::MAX_DEPTH;
  }
};

// a cross-section table with its grid, held by value (bf_heating.h BfhIntegrand)
struct PhixsGrid {
  int32_t npoints;
  double increment, last_nuovernuedge;
  const float *xs;
  AHD float at(const double nu_edge, const double nu) const {
    return artis::phixs_fromtable_grid(npoints, increment, last_nuovernuedge, xs, nu_edge, nu);
  }
};

// ---------------------------------------------------------------- the integrands (ratecoeff.cc:75-121)
// alpha_sp_integrand ratecoeff.cc:75, over nu_minus_nu_edge
template <class Math>
struct AlphaSpIntegrand {
  PhixsGrid g;
  double nu_edge;
  float T_e;
  AHD double operator()(const double nu_minus_nu_edge) const {
    const float sigma_bf = g.at(nu_edge, nu_minus_nu_edge + nu_edge);
    return (2 / artis::CLIGHTSQUARED) * sigma_bf * artis::pow2(nu_edge + nu_minus_nu_edge) * Math::exp(-artis::HOVERKB * nu_minus_nu_edge / T_e);
  }
};
// bfcooling_integrand ratecoeff.cc:115, over nu_minus_nu_edge
template <class Math>
struct BfcoolingIntegrand {
  PhixsGrid g;
  double nu_edge;
  float T_e;
  AHD double operator()(const double nu_minus_nu_edge) const {
    const float sigma_bf = g.at(nu_edge, nu_minus_nu_edge + nu_edge);
    return sigma_bf * nu_minus_nu_edge * (2 * artis::HPLANCK / artis::CLIGHTSQUARED) * (nu_minus_nu_edge + nu_edge) * (nu_minus_nu_edge + nu_edge) *
           Math::exp(-artis::HOVERKB * nu_minus_nu_edge / T_e);
  }
};
#if ARTIS_OPT_USE_LUT_PHOTOION
// gammacorr_integrand ratecoeff.cc:93, over nu; radfield::planck radfield.h:50 (physics.h:914) with the policy's expm1
template <class Math>
struct GammacorrIntegrand {
  PhixsGrid g;
  double nu_edge;
  float temperature;
  AHD double operator()(const double nu) const {
    const float sigma_bf = g.at(nu_edge, nu);
    const double planck = 2 * artis::HPLANCK * artis::pow3(nu) / artis::pow2(artis::CLIGHT) / Math::expm1(artis::HOVERKB * nu / temperature);
    return sigma_bf * (1. / artis::HPLANCK) / nu * planck * (1 - Math::exp(-artis::HOVERKB * nu / temperature));
  }
};
#endif

// ---------------------------------------------------------------- one continuum
// a continuum of the tables: level ul (unique index) and its target t; ul < 0: no entry of the reference's loops writes this row
struct Cont {
  int32_t ul, t;
};
// what an entry reads of its continuum (ratecoeff.cc:171-181)
struct ContConsts {
  double statw_lower, statw_upper, prob, nu_threshold, nu_max_phixs;
  PhixsGrid grid;
};
AHD ContConsts cont_consts(const DevModel &M, const Cont c) {
  const int ui = M.level_ion[c.ul];
  const int element = M.ion_element[ui];
  const int ion = ui - M.elem_uniqueionindexstart[element];
  const int level = c.ul - M.ion_uniquelevelindexstart[ui];
  ContConsts k;
  k.statw_lower = artis::statw(M, c.ul);
  k.statw_upper = artis::statw(M, artis::lstart(M, element, ion + 1) + artis::phixs_upperlevel(M, c.ul, c.t));
  k.prob = artis::phixs_probability(M, c.ul, c.t);
  const double E_threshold = artis::phixs_threshold(M, element, ion, level, c.t);
  k.nu_threshold = E_threshold / artis::HPLANCK;  // a division (ratecoeff.cc:179)
  k.nu_max_phixs = k.nu_threshold * M.last_phixs_nuovernuedge;
  k.grid = PhixsGrid{(int32_t)M.NPHIXSPOINTS, M.NPHIXSNUINCREMENT, M.last_phixs_nuovernuedge, artis::phixs_table(M, c.ul)};
  return k;
}
// modified_sahafact ratecoeff.cc:188
AHD double modified_sahafact(const ContConsts &k, const double Tpow_t, int32_t *flag) {
  const double v = artis::SAHACONST * k.statw_lower / k.statw_upper * Tpow_t;
  if (!(v >= 0.) || !isfinite(v)) *flag |= BAD_SAHAFACT;
  return v;
}
// the finished entries and the reference's asserts on them (ratecoeff.cc:198-225)
AHD double finish_alpha_or_cooling(const ContConsts &k, const double sahafact, const double integral, const int32_t bad, int32_t *flag) {
  const double v = FOURPI * sahafact * k.prob * integral;
  if (!(isfinite(v) && v >= 0)) *flag |= bad;
  return v;
}
AHD double finish_gammacorr(const ContConsts &k, double gammacorr, int32_t *flag) {
  gammacorr *= FOURPI * k.prob;
  if (!(gammacorr >= 0)) *flag |= BAD_GAMMACORR;
  return gammacorr;
}

// entry [cont][t] of table `kind` as the reference forms it: one gk61_integrate call
template <class Math>
AHD double rc_entry(const DevModel &M, const double *Tpow, const Cont cont, const int t, const int kind, int32_t *flag, Totals *tot) {
  const ContConsts k = cont_consts(M, cont);
  const auto temperature = static_cast<float>(M.temperature_grid[t]);
  double error = 0.;
  Gk61Stats st;
#if ARTIS_OPT_USE_LUT_PHOTOION
  if (kind == KIND_GAMMACORR) {
    const GammacorrIntegrand<Math> f{k.grid, k.nu_threshold, temperature};
    const double gammacorr = artis_bfh::gk61_integrate(f, k.nu_threshold, k.nu_max_phixs, EPSREL, &error, &st);
    tot->add(st);
    return finish_gammacorr(k, gammacorr, flag);
  }
#endif
  const double sahafact = modified_sahafact(k, Tpow[t], flag);
  double integral;
  if (kind == KIND_ALPHA_SP) {
    const AlphaSpIntegrand<Math> f{k.grid, k.nu_threshold, temperature};
    integral = artis_bfh::gk61_integrate(f, 0, k.nu_max_phixs - k.nu_threshold, EPSREL, &error, &st);
  } else {
    const BfcoolingIntegrand<Math> f{k.grid, k.nu_threshold, temperature};
    integral = artis_bfh::gk61_integrate(f, 0, k.nu_max_phixs - k.nu_threshold, EPSREL, &error, &st);
  }
  tot->add(st);
  return finish_alpha_or_cooling(k, sahafact, integral, kind == KIND_ALPHA_SP ? BAD_ALPHA_SP : BAD_BFCOOLING, flag);
}

// ---------------------------------------------------------------- the first node of N integrals over one interval
// integrate_non_adaptive_m1_1<61> (gausskronrod.h:173; bf_heating.h gk61_unit) of N integrands evaluated together: ev(slot, x) gives
// the N values at x, the rule's node `slot` (0: the centre; i: +x[i]; 30 + i: -x[i]). Each sum runs in the rule's order. The loops stay
// rolled on the device: unrolled, the kernel held 512 registers and spilled (one wave per SIMD).
constexpr int NSLOTS = 61;
template <int N>
struct Vals {
  double v[N];
};
template <int N, class Ev>
AHD void rc_unit(const Ev &ev, const GK61 &g, const double scale, const double mean, double *kr, double *error) {
  const Vals<N> fc = ev(0, (scale * 0.) + mean);
  double gr[N];
  for (int n = 0; n < N; n++) {
    kr[n] = fc.v[n] * g.w[0];
    gr[n] = 0.;
  }
#pragma unroll 1
  for (unsigned i = 1; i < 31; i += 2) {
    const Vals<N> fp = ev((int)i, (scale * g.x[i]) + mean);
    const Vals<N> fm = ev((int)(30 + i), (scale * -g.x[i]) + mean);
    for (int n = 0; n < N; n++) {
      kr[n] += (fp.v[n] + fm.v[n]) * g.w[i];
      gr[n] += (fp.v[n] + fm.v[n]) * g.wg[i / 2];
    }
  }
#pragma unroll 1
  for (unsigned i = 2; i < 31; i += 2) {
    const Vals<N> fp = ev((int)i, (scale * g.x[i]) + mean);
    const Vals<N> fm = ev((int)(30 + i), (scale * -g.x[i]) + mean);
    for (int n = 0; n < N; n++) kr[n] += (fp.v[n] + fm.v[n]) * g.w[i];
  }
  for (int n = 0; n < N; n++) error[n] = artis::dmax(fabs(kr[n] - gr[n]), fabs(kr[n] * 2.220446049250313e-16 * 2));
}
// the abscissa of node `slot` of the first node of [a, b], as rc_unit forms it (whoever stages the cross-sections forms the same bits)
AHD double rc_abscissa(const int slot, const double a, const double b) {
  const GK61 &g = artis_bfh::gk61_tables();
  const double mean = (b + a) / 2;
  const double scale = (b - a) / 2;
  if (slot == 0) return (scale * 0.) + mean;
  return (slot <= 30) ? (scale * g.x[slot]) + mean : (scale * -g.x[slot - 30]) + mean;
}

// the cross-section at a node: computed from the table here; the kernel may hand in a form that reads staged values by slot
struct SigmaComputed {
  PhixsGrid g;
  double nu_edge;
  AHD float alpha_cooling(const int slot, const double nu_minus_nu_edge) const { return g.at(nu_edge, nu_minus_nu_edge + nu_edge); }
  AHD float gammacorr(const int slot, const double nu) const { return g.at(nu_edge, nu); }
};

// alpha_sp_integrand and bfcooling_integrand at one abscissa from one cross-section and one exponential
template <class Math, class Sigma>
struct AlphaCoolingEval {
  Sigma sigma;
  double nu_edge;
  float T_e;
  AHD Vals<2> operator()(const int slot, const double nu_minus_nu_edge) const {
    const float sigma_bf = sigma.alpha_cooling(slot, nu_minus_nu_edge);
    const double nu = nu_minus_nu_edge + nu_edge;
    const double boltzmann = Math::exp(-artis::HOVERKB * nu_minus_nu_edge / T_e);
    Vals<2> out;
    out.v[0] = (2 / artis::CLIGHTSQUARED) * sigma_bf * artis::pow2(nu) * boltzmann;
    out.v[1] = sigma_bf * nu_minus_nu_edge * (2 * artis::HPLANCK / artis::CLIGHTSQUARED) * nu * nu * boltzmann;
    return out;
  }
};
#if ARTIS_OPT_USE_LUT_PHOTOION
template <class Math, class Sigma>
struct GammacorrEval {
  Sigma sigma;
  float temperature;
  AHD Vals<1> operator()(const int slot, const double nu) const {
    const float sigma_bf = sigma.gammacorr(slot, nu);
    const double planck = 2 * artis::HPLANCK * artis::pow3(nu) / artis::pow2(artis::CLIGHT) / Math::expm1(artis::HOVERKB * nu / temperature);
    Vals<1> out;
    out.v[0] = sigma_bf * (1. / artis::HPLANCK) / nu * planck * (1 - Math::exp(-artis::HOVERKB * nu / temperature));
    return out;
  }
};
#endif

// recursive_adaptive_integrate<61> at the root (abs_tol = 0) decided on a first node that is already there: the estimate when the node
// suffices (bf_heating.h gk61_adaptive), else false and the caller runs the whole integral through gk61_integrate
AHD bool first_node_suffices(const double scale, const double r1, const double err_local, double *estimate) {
  *estimate = scale * r1;
  const double abs_tol1 = fabs(*estimate * EPSREL);
  return !(abs_tol1 < err_local);
}

// the whole integral of table `kind` through gk61_integrate, for an integral whose first node asked to subdivide: one function, not
// inlined, so that the walk's per-depth arrays are not the kernel's
template <class Math>
ANOINLINE double rc_integrate_whole(const int kind, const PhixsGrid grid, const double nu_threshold, const double nu_max_phixs, const float temperature,
                                    Gk61Stats *st) {
  double error = 0.;
#if ARTIS_OPT_USE_LUT_PHOTOION
  if (kind == KIND_GAMMACORR) {
    const GammacorrIntegrand<Math> f{grid, nu_threshold, temperature};
    return artis_bfh::gk61_integrate(f, nu_threshold, nu_max_phixs, EPSREL, &error, st);
  }
#endif
  if (kind == KIND_ALPHA_SP) {
    const AlphaSpIntegrand<Math> f{grid, nu_threshold, temperature};
    return artis_bfh::gk61_integrate(f, 0, nu_max_phixs - nu_threshold, EPSREL, &error, st);
  }
  const BfcoolingIntegrand<Math> f{grid, nu_threshold, temperature};
  return artis_bfh::gk61_integrate(f, 0, nu_max_phixs - nu_threshold, EPSREL, &error, st);
}

// entry [cont][t] of the two or three tables, alpha_sp and bfcooling from shared evaluations: out[KIND_*] (gammacorr: +0 in builds
// without USE_LUT_PHOTOION); returns the entry's flag bits
template <class Math, class Sigma>
AHD int32_t rc_entry_shared_with(const DevModel &M, const double *Tpow, const ContConsts &k, const Sigma &sigma, const int t, double *out, Totals *tot) {
  int32_t flag = 0;
  const auto temperature = static_cast<float>(M.temperature_grid[t]);
  const GK61 &g = artis_bfh::gk61_tables();
  const Gk61Stats one{1, 0};
  Gk61Stats st;
  const double sahafact = modified_sahafact(k, Tpow[t], &flag);
  double integral[2];
  {
    const double a = 0, b = k.nu_max_phixs - k.nu_threshold;
    bool done[2] = {false, false};
    if (a < b) {
      double kr[2], err_local[2];
      const AlphaCoolingEval<Math, Sigma> ev{sigma, k.nu_threshold, temperature};
      const double scale = (b - a) / 2;
      rc_unit<2>(ev, g, scale, (b + a) / 2, kr, err_local);
      for (int n = 0; n < 2; n++)
        if ((done[n] = first_node_suffices(scale, kr[n], err_local[n], &integral[n]))) tot->add(one);
    }
    if (!done[0]) {
      integral[0] = rc_integrate_whole<Math>(KIND_ALPHA_SP, k.grid, k.nu_threshold, k.nu_max_phixs, temperature, &st);
      tot->add(st);
    }
    if (!done[1]) {
      integral[1] = rc_integrate_whole<Math>(KIND_BFCOOLING, k.grid, k.nu_threshold, k.nu_max_phixs, temperature, &st);
      tot->add(st);
    }
  }
  out[KIND_ALPHA_SP] = finish_alpha_or_cooling(k, sahafact, integral[0], BAD_ALPHA_SP, &flag);
  out[KIND_BFCOOLING] = finish_alpha_or_cooling(k, sahafact, integral[1], BAD_BFCOOLING, &flag);
  out[KIND_GAMMACORR] = 0.;
#if ARTIS_OPT_USE_LUT_PHOTOION
  {
    const double a = k.nu_threshold, b = k.nu_max_phixs;
    double gammacorr;
    bool done = false;
    if (a < b) {
      double kr[1], err_local[1];
      const GammacorrEval<Math, Sigma> ev{sigma, temperature};
      const double scale = (b - a) / 2;
      rc_unit<1>(ev, g, scale, (b + a) / 2, kr, err_local);
      if ((done = first_node_suffices(scale, kr[0], err_local[0], &gammacorr))) tot->add(one);
    }
    if (!done) {
      gammacorr = rc_integrate_whole<Math>(KIND_GAMMACORR, k.grid, k.nu_threshold, k.nu_max_phixs, temperature, &st);
      tot->add(st);
    }
    out[KIND_GAMMACORR] = finish_gammacorr(k, gammacorr, &flag);
  }
#endif
  return flag;
}
template <class Math>
AHD int32_t rc_entry_shared(const DevModel &M, const double *Tpow, const Cont cont, const int t, double *out, Totals *tot) {
  const ContConsts k = cont_consts(M, cont);
  const SigmaComputed sigma{k.grid, k.nu_threshold};
  return rc_entry_shared_with<Math>(M, Tpow, k, sigma, t, out, tot);
}

// ---- the arrays of a call: what the kernel (device pointers) and the x86 loops (host pointers) hand to the body below
struct Arrays {
  int64_t nitems;      // nbfcontinua x TABLESIZE
  const Cont *conts;   // [nbfcontinua]
  const double *Tpow;  // [TABLESIZE]
  double *spontrecomb, *corrphotoion, *bfcooling;  // [nbfcontinua][TABLESIZE]; corrphotoion null in builds without USE_LUT_PHOTOION
  int32_t *flags;                                  // [nbfcontinua][TABLESIZE]
};
AHD void store_item(const Arrays &A, const int64_t item, const double *v, const int32_t flag, Totals *tot) {
  A.spontrecomb[item] = v[KIND_ALPHA_SP];
  if (A.corrphotoion) A.corrphotoion[item] = v[KIND_GAMMACORR];
  A.bfcooling[item] = v[KIND_BFCOOLING];
  A.flags[item] = flag;
  tot->v[3] += flag != 0;
}
// item = continuum x TABLESIZE + temperature index (get_bflutindex ratecoeff.cc:123): every item has this one writer; a row the
// reference's loops do not reach is +0. shared: rc_entry_shared, else three rc_entry calls.
template <class Math>
AHD void item_entry(const DevModel &M, const Arrays &A, const int64_t item, const bool shared, Totals *tot) {
  const int64_t ci = item / TABLESIZE;
  const int t = (int)(item - ci * TABLESIZE);
  const Cont cont = A.conts[ci];
  double v[3] = {0., 0., 0.};
  int32_t flag = 0;
  if (cont.ul >= 0) {
    if (shared) {
      flag = rc_entry_shared<Math>(M, A.Tpow, cont, t, v, tot);
    } else {
      v[KIND_ALPHA_SP] = rc_entry<Math>(M, A.Tpow, cont, t, KIND_ALPHA_SP, &flag, tot);
      if (ARTIS_OPT_USE_LUT_PHOTOION) v[KIND_GAMMACORR] = rc_entry<Math>(M, A.Tpow, cont, t, KIND_GAMMACORR, &flag, tot);
      v[KIND_BFCOOLING] = rc_entry<Math>(M, A.Tpow, cont, t, KIND_BFCOOLING, &flag, tot);
    }
  }
  store_item(A, item, v, flag, tot);
}

// ---------------------------------------------------------------- host side (the model's arrays readable where this runs)
// Tpow[t] = std::pow(static_cast<float>(temperature_grid[t]), -1.5) (ratecoeff.cc:186-188), with the host's libm
inline void make_tpow(const double *temperature_grid, double *Tpow) {
  for (int t = 0; t < TABLESIZE; t++) {
    const auto temperature = static_cast<float>(temperature_grid[t]);
    Tpow[t] = std::pow(temperature, -1.5);
  }
}
// the rows the reference's loops write (ratecoeff.cc:148-173): ions 0 .. nions - 2 of every element, levels below nlevels_ionising,
// every target, at row level_bflist_start[ul] + target. False: a row outside [0, nbfcontinua), or a covered level without a
// cross-section table (level_phixsstart outside [0, nphixslevels): the reference asserts on an empty table, ratecoeff.cc:192).
inline bool list_continua(const int nelements, const int64_t nbfcontinua, const int64_t nphixslevels, const int32_t *elem_nions,
                          const int32_t *elem_uniqueionindexstart, const int32_t *ion_nlevels_ionising, const int32_t *ion_uniquelevelindexstart,
                          const int32_t *level_nphixstargets, const int32_t *level_bflist_start, const int32_t *level_phixsstart,
                          std::vector<Cont> &conts) {
  conts.assign((size_t)(nbfcontinua > 0 ? nbfcontinua : 0), Cont{-1, -1});
  for (int element = 0; element < nelements; element++)
    for (int ion = 0; ion < elem_nions[element] - 1; ion++) {
      const int ui = elem_uniqueionindexstart[element] + ion;
      for (int level = 0; level < ion_nlevels_ionising[ui]; level++) {
        const int ul = ion_uniquelevelindexstart[ui] + level;
        if (level_nphixstargets[ul] > 0 && (level_phixsstart[ul] < 0 || level_phixsstart[ul] >= nphixslevels)) return false;
        for (int t = 0; t < level_nphixstargets[ul]; t++) {
          const int64_t row = (int64_t)level_bflist_start[ul] + t;
          if (row < 0 || row >= nbfcontinua) return false;
          conts[(size_t)row] = Cont{ul, t};
        }
      }
    }
  return true;
}

}  // namespace artis_rc
