// initial_state.h -- the cells' state before the first timestep, per decay path and per cell.
//
// What the reference does between reading the model and its first update_grid: assign_initial_temperatures() (grid.cc:1077-1135) --
// the energy every decay path has released per mass of its top nuclide between t_model and tstart, every decay weighted by t' / tstart
// for the adiabatic loss since it happened (calc_energy_per_massoftopnuc_decaypath_withexpansion decay.cc:1086-1097, through the
// useexpansionfactor branch of calculate_decaychain decay.h:56-129), per cell the sequential sum over the paths
// (get_modelcell_endecay_per_mass decay.cc:1052-1062: packet_init.h cell_checkpoints without its stores) plus the model's initial
// energy, T_initial with its clamps, T_e = T_J = T_R = T_initial, W = 1 -- then the grey opacity (calculate_cell_kappagrey
// grid.cc:1864-1926, called at :2420 and, for JUST2022, again at update_grid.cc:603 with the first step's mass fractions, which is the
// value anything reads) and the first step's grey depth and thickness flag (update_grid.cc:606-627: deposition.h cell_grey_depth and
// cell_thickness, unchanged). The engine's kernels (stage_initial.h) and the loops of tests/initial_state_host (x86) call the same
// bodies.
//
// RPKT_GREY_TYPE is a RUNTIME value here (artis_initial_params.rpkt_grey_type), as the three switches of artis_packet_init_model: the
// stage runs once, and one library is tested all three ways.
//
// Floating-point discipline as decay_update.h: -ffp-contract=off, the reference's order of operations and float / double mixing.
#pragma once
#include <cmath>
#include <string>

#include "packet_init.h"

namespace artis_init {

constexpr double STEBO = 5.670400e-5;  // constants.h:41

// ---- the Bateman sum with the expansion factor (decay.h:56-129, useexpansionfactor; beside artis_decay::decaychain)

// lambdas[0 .. n): 1 / mean life along the path; the last one counts as 0 (calc_decaypath_unitfactor decay.cc:500-504, and the assert
// of decay.h:64). Term j is (exp(-x) + expm1(-x) / x) / denominator_j for x = lambda_j timediff > 0, else 0 (decay.h:99-102). The
// clamps are the reference's two (decay.h:124) and the one decaychain adds (the largest |term| times lambdaproduct below DBL_MIN).
// scale is measured in the summands BEFORE their cancellation: for small x, exp(-x) and expm1(-x) / x are each of size 1 and leave
// x / 2, so a term's rounding is eps / |denominator|, not eps |term|: scale = lambdaproduct max_j (x_j > 0 ? 1 / |denominator_j| : 0),
// x_dom the x of that j.
AHD artis_decay::Chain decaychain_expansion(const double *lambdas, const int n, const double timediff) {
  const auto lam = [&](int i) { return (i == n - 1) ? 0. : lambdas[i]; };
  double lambdaproduct = 1.;
  for (int j = 0; j < n - 1; j++) lambdaproduct *= lam(j);
  double sum = 0., maxabsterm = 0., maxinvdenom = 0., x_dom = 0.;
  for (int j = 0; j < n; j++) {
    const double lambda_j = lam(j);
    double denominator = 1.;
    for (int p = 0; p < n; p++)
      if (p != j) denominator *= (lam(p) - lambda_j);
    double sumterm = 0.;
    const double x = lambda_j * timediff;
    if (x > 0.) {
      sumterm = (exp(-x) + (expm1(-x) / x)) / denominator;
      const double invdenom = 1. / fabs(denominator);
      if (invdenom > maxinvdenom) {
        maxinvdenom = invdenom;
        x_dom = x;
      }
    }
    sum += sumterm;
    const double abssumterm = fabs(sumterm);
    maxabsterm = (abssumterm > maxabsterm) ? abssumterm : maxabsterm;
  }
  const double last = lambdaproduct * sum;
  artis_decay::Chain r{last, lambdaproduct * maxinvdenom, x_dom};
  if (last < 0. || fabs(sum) <= n * artis_decay::DBL_EPS * maxabsterm || lambdaproduct * maxabsterm < artis_decay::DBL_MINV) r.abund = 0.;
  return r;
}

// ---- per path

// calc_energy_per_massoftopnuc_decaypath_withexpansion decay.cc:1086-1097 for one path; *scale and *x_dom: the chain's
AHD double path_energy_expansion(const artis_pinit::Tables &T, const int p, const double tstart, double *scale, double *x_dom) {
  const int i0 = T.path_start[p], n = T.path_start[p + 1] - i0;
  const int top = T.path_nucindex[i0], last = T.path_nucindex[i0 + n - 2];
  const artis_decay::Chain ch = decaychain_expansion(T.path_lambda + i0, n, tstart - T.t_model);
  *scale = ch.scale;
  *x_dom = ch.x_dom;
  // get_decaypath_lastdecayenergy decay.cc:238-248, as packet_init.h path_energy forms it
  const double endecay = T.endecay_gamma[last] + T.endecay_particle[(int64_t)last * artis_pinit::NDECAYTYPES + T.path_last_decaytype[p]];
  const double lastdecayenergy = endecay / T.probsum[last];
  return T.path_branchproduct[p] * ch.abund * lastdecayenergy / T.nuc_mass[top];
}

// ---- per cell

// grid.cc:1110-1128: the non-finite test first, then the clamp at MINTEMP, then at MAXTEMP. *flag: the branch taken
AHD float initial_temperature(const float rho_tmin, const double endecay_per_mass, const double tmin, const double tstart, int32_t *flag) {
  float T_initial = static_cast<float>(pow(artis::CLIGHT / 4 / STEBO * artis::pow3(tmin / tstart) * rho_tmin * endecay_per_mass, 1. / 4.));
  *flag = ARTIS_INITIAL_INSIDE;
  if (!isfinite(T_initial)) {
    T_initial = ARTIS_OPT_MINTEMP;
    *flag = ARTIS_INITIAL_NONFINITE;
  } else if (T_initial < ARTIS_OPT_MINTEMP) {
    T_initial = ARTIS_OPT_MINTEMP;
    *flag = ARTIS_INITIAL_BELOW_MINTEMP;
  } else if (T_initial > ARTIS_OPT_MAXTEMP) {
    T_initial = ARTIS_OPT_MAXTEMP;
    *flag = ARTIS_INITIAL_ABOVE_MAXTEMP;
  }
  return T_initial;
}

// what the grey opacity is made from besides the cell (artis_initial_params)
struct Grey {
  int32_t type;
  double mfegroup, mtot_input;
  const float *ffegrp, *initelectronfrac;  // [cell]; null unless the type reads them
  const int32_t *elem_anumber;             // [nelements]
  int32_t nelements;
};

// grid.cc:1896-1903: the lanthanides' mass fraction of one cell, in element order; massfrac: the cell's [nelements]
AHD double lanthanide_massfrac(const Grey &G, const float *massfrac) {
  double X_lan = 0.;
  for (int element = 0; element < G.nelements; element++) {
    const int z = G.elem_anumber[element];
    if (z >= 57 && z <= 71) X_lan += massfrac[element];
  }
  return X_lan;
}

// calculate_cell_kappagrey grid.cc:1864-1926. massfrac: the cell's [nelements] (JUST2022). *flag gets ARTIS_INITIAL_KAPPA_INVALID
// where the reference asserts (:1923-1924)
AHD float cell_kappagrey(const Grey &G, const int64_t c, const float rho_tmin, const float T_R, const float *massfrac, int32_t *flag) {
  if (rho_tmin <= 0.) return 0.;
  double kappa = 0.;
  if (G.type == ARTIS_GREY_FEGROUP_APPROX) {
    constexpr double GREY_OP = 0.1;
    kappa = ((0.9 * G.ffegrp[c]) + 0.1) * GREY_OP / ((0.9 * G.mfegroup / G.mtot_input) + 0.1);
  } else if (G.type == ARTIS_GREY_TANAKA2020) {
    // pairs of (upper Ye limit, kappa [cm^2/g]), Tanaka et al. (2020) table 1
    const double limit[6] = {0.1, 0.15, 0.20, 0.25, 0.30, 0.35};
    const double value[6] = {19.5, 32.2, 22.3, 5.6, 5.36, 3.3};
    const float Ye = G.initelectronfrac[c];
    kappa = 0.96;
    for (int i = 0; i < 6; i++)
      if (Ye <= limit[i]) {
        kappa = value[i];
        break;
      }
  } else {
    const double T_rad = T_R;
    const double X_lan = lanthanide_massfrac(G, massfrac);
    if (X_lan < 1e-7) {
      kappa = 0.2;
    } else if (X_lan < 1e-3) {
      kappa = 3 * pow(X_lan / 1e-3, 0.3);
    } else if (X_lan < 1e-1) {
      kappa = 3 * pow(X_lan / 1e-3, 0.5);
    } else {
      kappa = 30 * pow(X_lan / 1e-1, 0.1);
    }
    if (T_rad < 2000.) {
      const double t = T_rad / 2000.;
      kappa *= (t * t) * (t * t) * t;  // pow5 constants.h:18-19
    }
  }
  const float kappa_float = static_cast<float>(kappa);
  if (!(kappa_float >= 0.f) || !isfinite(kappa_float)) *flag |= ARTIS_INITIAL_KAPPA_INVALID;
  return kappa_float;
}

// the per-cell inputs and the result block, every array [cell] but massfrac [cell][nelements]
struct CellIn {
  const float *rho_tmin, *rho, *massfrac;  // rho and massfrac: the decay update's at tstart
  const double *initenergyq;               // null: no initial-energy channel (grid.cc:1106)
  const double *radial_pos_tmin;
  double tmin, tstart;
};
struct CellOut {
  float *T_initial, *kappagrey, *grey_depth;
  double *endecay;
  int32_t *thick, *flags;
};

// one cell from its sum over the paths (grid.cc:1106-1134, then kappagrey and the thickness); returns the cell's flags
AHD int32_t cell_entry(const double paths_sum, const CellIn &in, const Grey &G, const artis_dep::Step &S, const int64_t c, const CellOut &out) {
  const double q = in.initenergyq ? in.initenergyq[c] : 0.;
  const double decayedenergy_per_mass = paths_sum + q;
  int32_t flag;
  const float T_initial = initial_temperature(in.rho_tmin[c], decayedenergy_per_mass, in.tmin, in.tstart, &flag);
  const float kappa = cell_kappagrey(G, c, in.rho_tmin[c], T_initial, in.massfrac + c * G.nelements, &flag);
  const float depth = artis_dep::cell_grey_depth(kappa, in.rho[c], in.radial_pos_tmin[c], S);
  out.endecay[c] = decayedenergy_per_mass;
  out.T_initial[c] = T_initial;
  out.kappagrey[c] = kappa;
  out.grey_depth[c] = depth;
  out.thick[c] = artis_dep::cell_thickness(depth, S);
  out.flags[c] = flag;
  return flag;
}

// ---- host: validation (plain C++)

// empty: the parameters are usable on ncell cells of a network whose snapshot time is t_model; else what is wrong with them
inline std::string initial_validate(const artis_initial_params &p, const int64_t ncell, const double t_model) {
  if (!std::isfinite(p.tstart) || !(p.tstart > 0.)) return "tstart is not positive and finite";
  if (p.tstart < t_model) return "tstart < t_model";
  if (std::isnan(p.optical_depth_is_thick) || (ARTIS_OPT_VPKT_ON && std::isnan(p.optical_depth_is_thick_vpkt))) return "optical_depth_is_thick is not a number";
  if (p.rpkt_grey_type == ARTIS_GREY_FEGROUP_APPROX) {
    if (ncell > 0 && !p.ffegrp) return "FEGROUP_APPROX needs ffegrp";
    if (!std::isfinite(p.mfegroup) || p.mfegroup < 0. || !std::isfinite(p.mtot_input) || !(p.mtot_input > 0.)) return "FEGROUP_APPROX needs mfegroup >= 0 and mtot_input > 0";
  } else if (p.rpkt_grey_type == ARTIS_GREY_TANAKA2020) {
    if (ncell > 0 && !p.initelectronfrac) return "TANAKA2020 needs initelectronfrac";
    for (int64_t c = 0; c < ncell; c++)
      if (!(p.initelectronfrac[c] > 0.f)) return "cell " + std::to_string(c) + ": TANAKA2020 with Ye <= 0";
  } else if (p.rpkt_grey_type != ARTIS_GREY_JUST2022) {
    return "unknown rpkt_grey_type " + std::to_string(p.rpkt_grey_type);
  }
  return "";
}

}  // namespace artis_init
