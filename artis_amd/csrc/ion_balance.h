// ion_balance.h -- partition functions and the ionisation balance of one cell (the LTE / nebular-approximation ion balance
// of the reference's grid update, ltepop.cc; element number densities grid.cc:1693-1730; the ions' total spontaneous
// recombination coefficients ratecoeff.cc:438, :643, :687-773).
//
// The engine's kernels (stage_ionbal.h) and the loops of tests/ionbal_host (x86) call the same per-element functions at the end
// of this file. Floating-point discipline as physics.h: -ffp-contract=off, and every expression
// keeps the reference's order of operations and its float/double mixing (partition functions, populations, n_e and the
// ion_alpha_sp table are floats; U is summed in double in level order; phi_saha's ratio of partition functions is a float
// quotient). The reference's assertions and log lines become flag bits (include/artis_amd.h ARTIS_IONBAL_*).
//
// Scope: builds without NLTE populations (no element has NLTE levels, NT_ON off): every population is LTE or Saha / rate
// balance, the level populations above the ground level are Boltzmann (calculate_levelpop_boltzmann ltepop.cc:395).
#pragma once
#include "radfield_fit.h"

#ifndef ARTIS_OPT_FORCE_SAHA_ION_BALANCE
#error "include/artis_options.h defines ARTIS_OPT_FORCE_SAHA_ION_BALANCE"
#endif

namespace artis_ib {

using artis::DevModel;
using artis::KB;
using artis::MH;
using artis::SAHACONST;
using artis::eps;
using artis::ionstage;
using artis::lstart;
using artis::statw;
using artis::uion;
constexpr double MINPOP = ARTIS_OPT_MINPOP;
constexpr int MAXIONS = 32;  // ions per element the per-cell solve holds (checked by the engine and the x86 build)

// per-cell flag bits (include/artis_amd.h)
constexpr int32_t NEUTRAL = ARTIS_IONBAL_NEUTRAL, MAXIT = ARTIS_IONBAL_MAXIT, PHI_OVERFLOW = ARTIS_IONBAL_PHI_OVERFLOW,
                  FRAC_ZEROED = ARTIS_IONBAL_FRAC_ZEROED, NOT_BRACKETED = ARTIS_IONBAL_NOT_BRACKETED,
                  INVALID_U = ARTIS_IONBAL_INVALID_U, NONFINITE = ARTIS_IONBAL_NONFINITE, FORCED_SAHA = ARTIS_IONBAL_FORCED_SAHA;
constexpr int32_t REFUSED = NOT_BRACKETED | INVALID_U | NONFINITE;  // a cell with one of these is not a usable state

// ---- element number densities (grid.cc:1693 get_elem_numberdens, :1719 set_nnetot)
AHD double elem_numberdens(const float massfrac, const float meanweight, const float rho) {
  return massfrac / static_cast<double>(meanweight) * rho;
}
AHD float nnetot(const DevModel &M, const float *massfrac, const float *meanweight, const float rho) {
  double nnetot = 0.;
  for (int element = 0; element < M.nelements; element++)
    nnetot += elem_numberdens(massfrac[element], meanweight[element], rho) * M.elem_anumber[element];
  return static_cast<float>(nnetot);
}

// get_groundlevelpop ltepop.h:75: the stored float, floored at MINPOP for a present element (0 for an absent one)
AHD double groundlevelpop(const float stored, const float massfrac) {
  const double nn = stored;
  if (nn < MINPOP) return massfrac > 0 ? MINPOP : 0.;
  return nn;
}

// ---- calculate_partfunct ltepop.cc:204 (levels above the ground level: calculate_levelpop_boltzmann :395)
AHD float partfunct(const DevModel &M, const int element, const int ion, const float ground_stored, const float massfrac,
                    const float T_exc, int32_t *flags) {
  // a ground population below MINPOP is replaced by 1 for the sum (it cancels but for the last bit)
  double nnground = groundlevelpop(ground_stored, massfrac);
  if (nnground < MINPOP) nnground = 1.;
  const int l0 = lstart(M, element, ion);
  const int nlevels = M.ion_nlevels[uion(M, element, ion)];
  const double groundpop = nnground;
  double U = 1.;
  for (int level = 1; level < nlevels; level++) {
    const double E_aboveground = eps(M, l0 + level) - eps(M, l0);
    const double nn = nnground * statw(M, l0 + level) / statw(M, l0) * exp(-E_aboveground / KB / T_exc);
    U += nn / groundpop;
  }
  U *= statw(M, l0);
  const float U_float = static_cast<float>(U);
  if (!(U_float > 0.f) || !isfinite(U_float)) *flags |= INVALID_U;
  return U_float;
}

// ---- the ions' spontaneous recombination coefficients
// get_groundcontindex atomic.h:122: the place of the ion's ground continuum in the ground-continuum list (input.cc:785-831),
// found by its edge; two ions with the same ground edge would take the first place (the reference's order of such ties is
// that of an unstable sort)
AHD int ion_groundcontindex(const DevModel &M, const int element, const int ion) {
  if (ion >= M.elem_nions[element] - 1) return -1;
  const int ul = lstart(M, element, ion);
  if (M.level_nphixstargets[ul] == 0) return -1;
  const double nu_edge = artis::phixs_threshold(M, element, ion, 0, 0) / artis::HPLANCK;
  for (int i = 0; i < M.nbfcontinua_ground; i++)
    if (M.groundcont_nu_edge[i] == nu_edge) return i;
  return -1;
}

// calculate_ionrecombcoeff(-1, T_e, element, upperion, {.assume_lte = true, .norm = TARGETLEVELPOP}) ratecoeff.cc:687-773:
// the entry of precalculate_ion_alpha_sp (ratecoeff.cc:438) for the ion below upperion
AHD double ionrecombcoeff_lte_targetpop(const DevModel &M, const float T_e, const int element, const int upperion) {
  if (upperion <= 0) return 0.;
  const int lowerion = upperion - 1;
  const float clumpednne = 1.F;
  const int nlevels_ionising_lower = M.ion_nlevels_ionising[uion(M, element, lowerion)];
  const int lowerstart = lstart(M, element, lowerion), upperstart = lstart(M, element, upperion);
  const auto alpha_level = [&](const int lower, const int t) -> double {
    return artis::rad_recomb(M, T_e, clumpednne, element, upperion, lower, t) / clumpednne;
  };
  double alpha = 0.;
  for (int lower = 0; lower < nlevels_ionising_lower; lower++) {
    const int ul = lowerstart + lower;
    const int nphixstargets = M.level_nphixstargets[ul];
    if (nphixstargets == 1) {
      alpha += alpha_level(lower, 0);
      continue;
    }
    // the Boltzmann weights of several targets relative to the lowest-energy one
    double E_ref = artis_rf::DBL_MAXV;
    for (int t = 0; t < nphixstargets; t++) {
      const double E = eps(M, upperstart + artis::phixs_upperlevel(M, ul, t));
      E_ref = (E < E_ref) ? E : E_ref;
    }
    double alpha_weighted = 0.;
    double weight_sum = 0.;
    for (int t = 0; t < nphixstargets; t++) {
      const int upper = upperstart + artis::phixs_upperlevel(M, ul, t);
      const double weight = statw(M, upper) * exp(-(eps(M, upper) - E_ref) / KB / T_e);
      alpha_weighted += weight * alpha_level(lower, t);
      weight_sum += weight;
    }
    if (weight_sum > 0.) alpha += alpha_weighted / weight_sum;
  }
  return alpha;
}

// get_ion_spontrecombcoeff ratecoeff.cc:643 on the float table [nions][TABLESIZE]
AHD double ion_spontrecombcoeff(const DevModel &M, const float *ion_alpha_sp, const int uniqueionindex, const float T_e) {
  const float *row = ion_alpha_sp + ((int64_t)uniqueionindex * ARTIS_OPT_TABLESIZE);
  const int upperindex = artis::temperature_upperindex(M, T_e);
  if (upperindex == 0) return row[0];
  if (upperindex < ARTIS_OPT_TABLESIZE) {
    const double T_lower = M.temperature_grid[upperindex - 1];
    const double T_upper = M.temperature_grid[upperindex];
    const double f_lower = row[upperindex - 1];
    const double f_upper = row[upperindex];
    return f_lower + ((f_upper - f_lower) / (T_upper - T_lower) * (T_e - T_lower));
  }
  return row[ARTIS_OPT_TABLESIZE - 1];
}

// ---- phi = N_ion / (N_ion+1 * nne): neither form depends on nne, so the engine forms them once per (cell, ion)
// phi_saha ltepop.cc:59
AHD double phi_saha(const DevModel &M, const int element, const int ion, const float U_ion, const float U_upperion, const float T_e) {
  const double ionpot = eps(M, lstart(M, element, ion + 1)) - eps(M, lstart(M, element, ion));
  const double partfunct_ratio = U_ion / U_upperion;
  return partfunct_ratio * SAHACONST * pow(static_cast<double>(T_e), -1.5) * exp(ionpot / KB / T_e);  // std::pow(float, double)
}
// phi_rate_balance ltepop.cc:73 (no collisional recombination, no non-thermal ionisation): gamma_ground is the ion's entry of
// the normalised gamma estimator (0 without a ground continuum)
AHD double phi_rate_balance(const DevModel &M, const float *ion_alpha_sp, const int element, const int ion, const float U_ion,
                            const float T_e, const float clumpfactor, const double gamma_ground) {
  const double Gamma_ion = gamma_ground * statw(M, lstart(M, element, ion)) / U_ion;
  const double Alpha_sp = ion_spontrecombcoeff(M, ion_alpha_sp, uion(M, element, ion), T_e);
  const double Col_rec = 0.;
  const double gamma_nt = 0.;
  return clumpfactor * (Alpha_sp + Col_rec) / (Gamma_ion + gamma_nt);
}
AHD bool use_phi_saha(const bool force_saha) { return force_saha || ARTIS_OPT_FORCE_SAHA_ION_BALANCE; }

// ---- one cell
struct Cell {
  float rho;
  const float *massfrac;    // [nelements]
  const float *meanweight;  // [nelements] (the cell's elem_meanweight, or the model's elem_meannucmass)
  const float *U;           // [nions] partition functions
  const double *phi;        // [nions] phi of every ion below an element's top ion (Saha or rate balance, as the cell uses)
  const double *gamma;      // [nbfcontinua_ground] the cell's normalised gamma estimator
  const int32_t *gci;       // [nions] ion_groundcontindex
  int32_t *uppermost;       // [nelements] out
};

// iongamma_is_zero ratecoeff.cc:883 (an element without NLTE levels)
AHD bool iongamma_is_zero(const DevModel &M, const Cell &c, const int element, const int ion) {
  if (ion >= M.elem_nions[element] - 1) return true;
  const int g = c.gci[uion(M, element, ion)];
  if (g < 0) return true;
  return c.gamma[g] == 0;
}

// find_uppermost_ion ltepop.cc:308
AHD int find_uppermost_ion(const DevModel &M, const Cell &c, const int element, const double nne_hi, const bool force_saha,
                           int32_t *flags) {
  const int nions = M.elem_nions[element];
  if (nions == 0) return -1;
  int uppermost_ion = nions - 1;
  if (!use_phi_saha(force_saha)) {
    for (int ion = 0; ion < nions - 1; ion++) {
      if (iongamma_is_zero(M, c, element, ion)) {
        uppermost_ion = ion;
        break;
      }
    }
  }
  double pop_ratio_ground_to_upper = 1.;
  for (int ion = 0; ion < uppermost_ion; ion++) {
    pop_ratio_ground_to_upper *= nne_hi * c.phi[uion(M, element, ion)];
    if (!isfinite(pop_ratio_ground_to_upper)) {
      *flags |= PHI_OVERFLOW;
      return ion;
    }
  }
  return uppermost_ion;
}

// calculate_ionfractions ltepop.cc:357 into frac[0..uppermost]; returns uppermost (-1: none)
AHD int ionfractions(const DevModel &M, const Cell &c, const int element, const double nne, double *frac, int32_t *flags) {
  const int uppermost_ion = c.uppermost[element];
  if (uppermost_ion < 0) return -1;
  frac[uppermost_ion] = 1;
  double normfactor = 1.;
  for (int ion = uppermost_ion - 1; ion >= 0; ion--) {
    frac[ion] = frac[ion + 1] * nne * c.phi[uion(M, element, ion)];
    normfactor += frac[ion];
  }
  for (int ion = 0; ion <= uppermost_ion; ion++) {
    frac[ion] = frac[ion] / normfactor;
    if (normfactor == 0. || !isfinite(frac[ion])) {
      *flags |= FRAC_ZEROED;
      frac[ion] = 0;
    }
  }
  return uppermost_ion;
}

// nne_solution_f ltepop.cc:142
AHD double nne_residual(const DevModel &M, const Cell &c, const double nne_assumed, int32_t *flags) {
  double nne_after = 0.;
  double frac[MAXIONS];
  for (int element = 0; element < M.nelements; element++) {
    const double nnelement = elem_numberdens(c.massfrac[element], c.meanweight[element], c.rho);
    if (nnelement > 0 && M.elem_nions[element] > 0) {
      const int uppermost_ion = ionfractions(M, c, element, nne_assumed, frac, flags);
      for (int ion = 0; ion <= uppermost_ion; ion++) {
        const double nnion = nnelement * frac[ion];
        const int ioncharge = ionstage(M, element, ion) - 1;
        nne_after += ioncharge * nnion;
      }
      if (!isfinite(nne_after)) *flags |= NONFINITE;
    }
  }
  nne_after = (MINPOP > nne_after) ? MINPOP : nne_after;  // std::max(MINPOP, nne_after)
  return nne_after - nne_assumed;
}

struct NneResidual {
  const DevModel *M;
  const Cell *c;
  int32_t *flags;
  AHD double operator()(const double nne) const { return nne_residual(*M, *c, nne, flags); }
};

// find_converged_nne ltepop.cc:282: the TOMS 748 root in [0, nne_max], its bracket's midpoint as a float. *evals: evaluations
// of the residual (the two ends included)
constexpr int NNE_MAXIT = 50;
AHD float find_converged_nne(const DevModel &M, const Cell &c, const double nne_max, int32_t *flags, int *evals) {
  const NneResidual f{&M, &c, flags};
  constexpr double nne_min = 0.;
  const double f_nne_min = f(nne_min);
  const double f_nne_max = f(nne_max);
  *evals = 2;
  if (!(f_nne_min * f_nne_max <= 0.)) {
    *flags |= NOT_BRACKETED;
    return 0.f;
  }
  int iter = NNE_MAXIT;
  const artis_rf::RootPair r = artis_rf::toms748(f, nne_min, nne_max, f_nne_min, f_nne_max, artis_rf::RelTol{1e-3}, &iter);
  *evals += iter;
  const double nne_solution = 0.5 * (r.lo + r.hi);
  if (iter >= NNE_MAXIT) *flags |= MAXIT;
  if (!isfinite(nne_solution)) *flags |= NONFINITE;
  return static_cast<float>((MINPOP > nne_solution) ? MINPOP : nne_solution);
}

// set_groundlevelpops ltepop.cc:433 of one element into ground[ion] (the element's entries)
AHD void set_groundlevelpops(const DevModel &M, const Cell &c, const int element, const float nne, float *ground, int32_t *flags) {
  const int nions = M.elem_nions[element];
  if (nions <= 0) return;
  const double nnelement = elem_numberdens(c.massfrac[element], c.meanweight[element], c.rho);
  double frac[MAXIONS];
  const int uppermost_ion = (nnelement > 0) ? ionfractions(M, c, element, nne, frac, flags) : -1;
  for (int ion = 0; ion < nions; ion++) {
    double nnion;
    if (nnelement <= 0) {
      nnion = 0.;
    } else if (ion <= uppermost_ion) {
      const double x = nnelement * frac[ion];
      nnion = (MINPOP > x) ? MINPOP : x;
    } else {
      nnion = MINPOP;
    }
    const int ui = uion(M, element, ion);
    ground[ui] = static_cast<float>(nnion * statw(M, lstart(M, element, ion)) / c.U[ui]);
  }
}

// set_groundlevelpops_neutral ltepop.cc:254
AHD void set_groundlevelpops_neutral(const DevModel &M, const Cell &c, float *ground) {
  for (int element = 0; element < M.nelements; element++) {
    const double nnelement = elem_numberdens(c.massfrac[element], c.meanweight[element], c.rho);
    for (int ion = 0; ion < M.elem_nions[element]; ion++) {
      double nnion;
      if (ion == 0) {
        nnion = nnelement;
      } else if (nnelement > 0.) {
        nnion = MINPOP;
      } else {
        nnion = 0.;
      }
      const int ui = uion(M, element, ion);
      ground[ui] = static_cast<float>(nnion * statw(M, lstart(M, element, ion)) / c.U[ui]);
    }
  }
}

// set_calculated_nne ltepop.cc:242 from the stored float populations (get_element_nne_contrib :128, get_nnion ltepop.h:106)
AHD float calculated_nne(const DevModel &M, const Cell &c, const float *ground) {
  double nne = 0.;
  for (int element = 0; element < M.nelements; element++) {
    if (elem_numberdens(c.massfrac[element], c.meanweight[element], c.rho) <= 0.) continue;
    double contrib = 0.;
    for (int ion = 0; ion < M.elem_nions[element]; ion++) {
      const int ui = uion(M, element, ion);
      const double nnion = groundlevelpop(ground[ui], c.massfrac[element]) * c.U[ui] / statw(M, lstart(M, element, ion));
      const int ioncharge = ionstage(M, element, ion) - 1;
      contrib += ioncharge * nnion;
    }
    nne += contrib;
  }
  return static_cast<float>((MINPOP > nne) ? MINPOP : nne);
}

// calculate_ion_balance_nne ltepop.cc:475: the uppermost ions, n_e, the ground populations ground[nions] and the final n_e.
// *nne_root: the root search's float (0 for the neutral fallback); *evals: residual evaluations.
AHD float ion_balance_nne(const DevModel &M, const Cell &c, const bool force_saha, float *ground, float *nne_root, int *evals,
                          int32_t *flags) {
  const double nne_max = c.rho / MH;
  bool only_lowest_ionstage = true;
  for (int element = 0; element < M.nelements; element++) {
    if (c.massfrac[element] > 0) {
      const int uppermost_ion = find_uppermost_ion(M, c, element, nne_max, force_saha, flags);
      c.uppermost[element] = uppermost_ion;
      only_lowest_ionstage = only_lowest_ionstage && (uppermost_ion <= 0);
    } else {
      c.uppermost[element] = M.elem_nions[element] - 1;
    }
  }
  *evals = 0;
  *nne_root = 0.f;
  if (only_lowest_ionstage) {
    *flags |= NEUTRAL;
    set_groundlevelpops_neutral(M, c, ground);
  } else {
    const float nne_solution = find_converged_nne(M, c, nne_max, flags, evals);
    *nne_root = nne_solution;
    if (*flags & REFUSED) return 0.f;
    for (int element = 0; element < M.nelements; element++) set_groundlevelpops(M, c, element, nne_solution, ground, flags);
  }
  return calculated_nne(M, c, ground);
}

// ---- one output element each: the bodies of the engine's kernels (stage_ionbal.h) and of the loops of tests/ionbal_host.
// Whoever calls them keeps one writer per element; a cell's flags are ORed by the caller where several entries share them.

// unique ion index -> (element, ion of the element)
struct IonOf {
  int element, ion;
};
AHD IonOf ion_of(const DevModel &M, const int ui) {
  const int element = M.ion_element[ui];
  return {element, ui - M.elem_uniqueionindexstart[element]};
}

// entry [ui][tempindex] of the ion_alpha_sp table (0 for an element's top ion: nothing recombines into it from above); the
// entry of tempindex 0 also writes the ion's ground-continuum index
AHD void alpha_sp_entry(const DevModel &M, const int ui, const int tempindex, float *alpha_sp, int32_t *gci) {
  const IonOf k = ion_of(M, ui);
  float v = 0.f;
  if (k.ion < M.elem_nions[k.element] - 1) {
    const auto T_e = static_cast<float>(M.temperature_grid[tempindex]);
    v = static_cast<float>(ionrecombcoeff_lte_targetpop(M, T_e, k.element, k.ion + 1));
  }
  alpha_sp[(int64_t)ui * ARTIS_OPT_TABLESIZE + tempindex] = v;
  if (tempindex == 0) gci[ui] = ion_groundcontindex(M, k.element, k.ion);
}

// the per-cell arrays of the set-up and the solve: inputs [ncell] and [ncell][nelements | nions | nbfg], then what solve_cell
// writes (flags: seeded by cell_setup, ORed into by the partition functions)
struct CellArrays {
  const float *rho, *massfrac, *meanweight_cell, *meanweight_model;  // meanweight_cell null: the model's elem_meannucmass
  const float *U;
  const double *phi, *gamma;
  const int32_t *gci;
  int32_t nbfg;
  int32_t *uppermost, *flags, *evals;
  float *ground, *nne, *nne_root;
};
AHD const float *cell_meanweight(const DevModel &M, const CellArrays &a, const int64_t c) {
  return a.meanweight_cell ? a.meanweight_cell + c * M.nelements : a.meanweight_model;
}

// the set-up of cell c: its T_e (the fit's or the host's; in a cell the fit has fitted -- fit_flags, null without a fit -- the
// host's override Te_override, null without one), nnetot, and the flags' seed: FORCED_SAHA or nothing
AHD void cell_setup(const DevModel &M, const int64_t c, const CellArrays &a, const float *Te_in, const float *Te_override,
                    const int32_t *fit_flags, const bool forced_saha, float *Te, float *nnetot_out) {
  float T = Te_in[c];
  if (fit_flags && Te_override && (fit_flags[c] & ARTIS_RADFIELD_FITTED)) T = Te_override[c];
  Te[c] = T;
  nnetot_out[c] = nnetot(M, a.massfrac + c * M.nelements, cell_meanweight(M, a, c), a.rho[c]);
  a.flags[c] = forced_saha ? FORCED_SAHA : 0;
}
// an LTE iteration and a THICK cell are balanced with forced Saha: the cells the radiation-field fit does not fit
AHD bool cell_forced_saha(const int32_t lte_iteration, const int32_t thick) { return !artis_rf::cell_is_fitted(lte_iteration, thick); }

// entry of the normalised gamma estimator (update_grid.cc:358) from the raw one and its cell's volume and timestep
AHD double gamma_normed_entry(const double gamma_raw, const double assocvolume_tmin, const double prev_mid, const double tmin,
                              const double deltat, const int32_t nprocs) {
  double estimator_normfactor, over4pi;
  artis_rf::cell_normfactors(assocvolume_tmin, prev_mid, tmin, deltat, nprocs, &estimator_normfactor, &over4pi);
  return gamma_raw * (estimator_normfactor / artis_rf::H);
}

// U[c][ui] from the current ground populations; *flags gets INVALID_U
AHD void partfunct_entry(const DevModel &M, const int64_t c, const int ui, const float *TJ, const float *Te, const float *ground_cur,
                         const float *massfrac, float *U, int32_t *flags) {
  const IonOf k = ion_of(M, ui);
  const float T_exc = ARTIS_OPT_LTEPOP_EXCITATION_USE_TJ ? TJ[c] : Te[c];
  const int64_t i = c * M.nions + ui;
  U[i] = partfunct(M, k.element, k.ion, ground_cur[i], massfrac[c * M.nelements + k.element], T_exc, flags);
}

// phi[c][ui]: 0 for an element's top ion, else Saha or rate balance as the cell's flags (FORCED_SAHA) and the build say
AHD void phi_entry(const DevModel &M, const int64_t c, const int ui, const int32_t cell_flags, const float *U, const float *Te,
                   const float *clump, const float *alpha_sp, const int32_t *gci, const double *gamma, const int nbfg, double *phi) {
  const IonOf k = ion_of(M, ui);
  const int64_t i = c * M.nions + ui;
  double p = 0.;
  if (k.ion < M.elem_nions[k.element] - 1) {
    if (use_phi_saha((cell_flags & FORCED_SAHA) != 0)) {
      p = phi_saha(M, k.element, k.ion, U[i], U[i + 1], Te[c]);
    } else {
      const int g = gci[ui];
      p = phi_rate_balance(M, alpha_sp, k.element, k.ion, U[i], Te[c], clump[c], g >= 0 ? gamma[c * nbfg + g] : 0.);
    }
  }
  phi[i] = p;
}

// cell c from its U, phi and flags so far: uppermost ions, the n_e root, ground populations, n_e, evaluations, flags. A cell that
// is REFUSED (before or by the solve) gets zero ground populations; one refused before it has no uppermost ions either (-1).
AHD void solve_cell(const DevModel &M, const int64_t c, const CellArrays &a) {
  int32_t flags = a.flags[c];
  const Cell cell{a.rho[c], a.massfrac + c * M.nelements, cell_meanweight(M, a, c), a.U + c * M.nions, a.phi + c * M.nions,
                  a.gamma + c * a.nbfg, a.gci, a.uppermost + c * M.nelements};
  float nne_root = 0.f;
  int evals = 0;
  float nne = 0.f;
  float *ground = a.ground + c * M.nions;
  if (flags & REFUSED) {  // an invalid partition function: nothing to balance
    for (int i = 0; i < M.nions; i++) ground[i] = 0.f;
    for (int e = 0; e < M.nelements; e++) cell.uppermost[e] = -1;
  } else {
    nne = ion_balance_nne(M, cell, (flags & FORCED_SAHA) != 0, ground, &nne_root, &evals, &flags);
    if (flags & REFUSED)
      for (int i = 0; i < M.nions; i++) ground[i] = 0.f;
  }
  a.nne[c] = nne;
  a.nne_root[c] = nne_root;
  a.evals[c] = evals;
  a.flags[c] = flags;
}

}  // namespace artis_ib
