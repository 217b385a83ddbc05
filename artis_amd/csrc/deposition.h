// deposition.h -- the deposition rates and the thickness flags of the grid update, per (nuclide, power vector), per cell and per
// timestep total.
//
// What the reference does with the decay coefficients of a timestep besides the composition: the analytic emission power of every
// source nuclide in five channels (gamma, positron, electron, alpha, spontaneous fission: calc_ana_emission_power_per_mass
// decay.cc:1105-1156) and the six qdot vectors (calc_qdot_power_per_mass decay.cc:1160); per cell the five analytic emission rates
// (get_modelcell_decaypower_per_mass decay.cc:1173), the normalised deposition estimators (normalise_deposition_estimators
// sn3d.cc:532-563), the deposition rate density of the non-thermal leptons (calculate_deposition_rate_density nonthermal.cc:2340)
// and the grey depth with the thickness flag of the next step's packets (update_grid.cc:606-627); per timestep the totals that
// deposition.out prints (sn3d.cc:240-286, :547-550). The engine's kernels (stage_deposition.h) and the loops of
// tests/deposition_host (x86) call the same bodies.
//
// Every sum here is a chain of dependent additions in the reference's order. Which paths add to a nuclide's power -- the paths whose
// top it is, in path order -- is built once on the host (build_dep_rows), next to the radioactive nuclides in index order: a stable
// nuclide's powers are exactly +0.0 and every path's top is radioactive, X and the energies are finite and non-negative, so a walk
// over the radioactive nuclides alone adds the same numbers to the same non-negative running sums.
//
// Floating-point discipline as decay_update.h: -ffp-contract=off, the reference's order of operations and float / double mixing.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "decay_update.h"

namespace artis_dep {

// nuclides whose X lines a lane has in flight before it adds the first of them (k_dep_cells: 32 lines of 256 B per wave)
constexpr int DEP_DEPTH = 32;

// the power vectors: five emission channels, then qdot of the six decay types in ARTIS_DECAYTYPE_* order
enum { CH_GAMMA = 0, CH_POSITRON = 1, CH_ELECTRON = 2, CH_ALPHA = 3, CH_SPFISSION = 4, NCHANNELS = 5, NQDOT = 6, NVECTORS = 11 };
// the timestep totals: the four cell sums {gamma, positron, electron, alpha}_dep [erg], then the vectors' products with totmassnuclide
enum { NCELLSUMS = 4, NTOTALS = NCELLSUMS + NVECTORS };

// ---- tables: a view of host or device arrays

struct Tables {
  int32_t nnuclides, npaths, nrad;
  const double *nuc_meanlife, *nuc_mass;  // [nnuclides] seconds (<= 0: stable); A * MH
  const double *energy;                   // [NVECTORS][nnuclides] energy per decay [erg] of every vector (times the branch probability)
  // nuclide n is the top of the paths top_path[top_start[n] .. top_start[n + 1]), in path order; top_end: their end nuclides
  const int32_t *top_start, *top_path, *top_end;
  const int32_t *rad_nuc;  // [nrad] the nuclides with meanlife > 0, in index order
};

// decay.cc:1116
AHD double power_per_currentmass(const Tables &T, const int v, const int nuc) {
  const double meanlife = T.nuc_meanlife[nuc];
  return (meanlife > 0.) ? T.energy[(int64_t)v * T.nnuclides + nuc] / meanlife / T.nuc_mass[nuc] : 0.;
}

// one entry of a power vector (decay.cc:1117-1125): the nuclide's own surviving share, then its paths in path order
AHD double power_entry(const Tables &T, const double *endnuc_coeff, const double *survivingfrac, const int v, const int nuc) {
  double p = power_per_currentmass(T, v, nuc) * survivingfrac[nuc];
  for (int k = T.top_start[nuc]; k < T.top_start[nuc + 1]; k++) p += power_per_currentmass(T, v, T.top_end[k]) * endnuc_coeff[T.top_path[k]];
  return p;
}

// ---- per cell. X is [nuclide][cell] (stride cells per nuclide), float; pw is [nrad][NCHANNELS]: the five powers of the radioactive
// nuclides, packed in the order of the walk

// decay.cc:1173 for the five channels at once: every X value is loaded once and feeds five chains. The loads of DEP_DEPTH nuclides
// are issued before their additions.
AHD void cell_power_sums(const Tables &T, const double *pw, const float *X, const int64_t stride, const int64_t c, double sum[NCHANNELS]) {
  for (int ch = 0; ch < NCHANNELS; ch++) sum[ch] = 0.;
  int k = 0;
  for (; k + DEP_DEPTH <= T.nrad; k += DEP_DEPTH) {
    float x[DEP_DEPTH];
#pragma unroll
    for (int j = 0; j < DEP_DEPTH; j++) x[j] = X[(int64_t)T.rad_nuc[k + j] * stride + c];
#pragma unroll
    for (int j = 0; j < DEP_DEPTH; j++) {
      const double xd = (double)x[j];
      const double *p = pw + (int64_t)(k + j) * NCHANNELS;
      for (int ch = 0; ch < NCHANNELS; ch++) sum[ch] += p[ch] * xd;
    }
  }
  for (; k < T.nrad; k++) {
    const double xd = (double)X[(int64_t)T.rad_nuc[k] * stride + c];
    const double *p = pw + (int64_t)k * NCHANNELS;
    for (int ch = 0; ch < NCHANNELS; ch++) sum[ch] += p[ch] * xd;
  }
}

// the same sums over EVERY nuclide from the vectors themselves [NVECTORS][nnuclides] (the restatement the tests hold the walk
// over the radioactive nuclides against)
AHD void cell_power_sums_all(const Tables &T, const double *vectors, const float *X, const int64_t stride, const int64_t c, double sum[NCHANNELS]) {
  for (int ch = 0; ch < NCHANNELS; ch++) {
    double s = 0.;
    for (int nuc = 0; nuc < T.nnuclides; nuc++) s += vectors[(int64_t)ch * T.nnuclides + nuc] * (double)X[(int64_t)nuc * stride + c];
    sum[ch] = s;
  }
}

// what a timestep's update works with besides the tables
struct Step {
  double t_mid, tmin, rmax;           // of the decay update: the next step's middle
  double prev_mid, prev_width;        // of the step just propagated
  int32_t nprocs, nts_next, num_grey_timesteps;
  double optical_depth_is_thick, optical_depth_is_thick_vpkt;
};

// the raw estimators {gamma, positron, electron, alpha} of cell c: raw[k][c * est_stride]
struct Estimators {
  const double *raw[NCELLSUMS];
  int32_t est_stride;
};

// the result block, every array [..][cell]
struct CellOut {
  double *eps_ana;  // [NCHANNELS][ncell]
  double *dep;      // [NCHANNELS][ncell]
  double *ntlepton;
  float *grey_depth;
  int32_t *thick;
};

// sn3d.cc:544, :553
AHD double estimator_normfactor(const double assocvolume_tmin, const Step &S) {
  const double r = S.prev_mid / S.tmin;
  const double dV = assocvolume_tmin * (r * r * r);
  return 1 / dV / S.prev_width / S.nprocs;
}

// update_grid.cc:606-612
AHD float cell_grey_depth(const float kappagrey, const float rho, const double radial_pos_tmin, const Step &S) {
  const double tratmid = S.t_mid / S.tmin;
  const double radial_pos = radial_pos_tmin * tratmid;
  const double d = (S.rmax * tratmid) - radial_pos;
  const double dist_to_obs = d > 0. ? d : 0.;
  return (float)(kappagrey * rho * dist_to_obs);
}

// update_grid.cc:619-627
AHD int32_t cell_thickness(const float grey_depth, const Step &S) {
  if ((grey_depth >= S.optical_depth_is_thick) && (S.nts_next < S.num_grey_timesteps)) return ARTIS_CELL_THICK;
  if (ARTIS_OPT_VPKT_ON && (grey_depth > S.optical_depth_is_thick_vpkt)) return ARTIS_CELL_THICK_VPKT_ONLY;
  return ARTIS_CELL_THIN;
}

// one cell from its five power sums (nonthermal.cc:2340-2380 and the thickness)
AHD void cell_entry(const double sum[NCHANNELS], const Step &S, const Estimators &E, const float *rho, const float *kappagrey,
                    const double *assocvolume_tmin, const double *radial_pos_tmin, const int64_t ncell, const int64_t c, const CellOut &out) {
  const double rho_c = rho[c];
  double eps[NCHANNELS], dep[NCHANNELS];
  for (int ch = 0; ch < NCHANNELS; ch++) eps[ch] = rho_c * sum[ch];
  const double normfactor = estimator_normfactor(assocvolume_tmin[c], S);
  const int64_t e = c * E.est_stride;
  dep[CH_GAMMA] = E.raw[0][e] * normfactor;
  if (ARTIS_OPT_PARTICLE_THERMALISATION_SCHEME == ARTIS_PARTICLE_INSTANTFULLDEPOSITION) {
    dep[CH_POSITRON] = eps[CH_POSITRON];
    dep[CH_ELECTRON] = eps[CH_ELECTRON];
    dep[CH_ALPHA] = eps[CH_ALPHA];
  } else {
    dep[CH_POSITRON] = E.raw[1][e] * normfactor;
    dep[CH_ELECTRON] = E.raw[2][e] * normfactor;
    dep[CH_ALPHA] = E.raw[3][e] * normfactor;
  }
  dep[CH_SPFISSION] = eps[CH_SPFISSION];
  const float depth = cell_grey_depth(kappagrey[c], rho[c], radial_pos_tmin[c], S);
  const int32_t thick = cell_thickness(depth, S);
  for (int ch = 0; ch < NCHANNELS; ch++) {
    out.eps_ana[ch * ncell + c] = eps[ch];
    out.dep[ch * ncell + c] = dep[ch];
  }
  out.ntlepton[c] = (dep[CH_GAMMA] + dep[CH_POSITRON] + dep[CH_ELECTRON]);
  out.grey_depth[c] = depth;
  out.thick[c] = thick;
}

// ---- the chains of the totals: term i of chain k; a chain is the sequential sum of its terms from +0.0

// sn3d.cc:547-550 (k < NCELLSUMS, i a cell) and sn3d.cc:267-273 (vector k - NCELLSUMS, i a nuclide)
AHD int64_t total_length(const Tables &T, const int64_t ncell, const int k) { return k < NCELLSUMS ? ncell : T.nnuclides; }
AHD double total_term(const Tables &T, const Estimators &E, const int32_t nprocs, const double *vectors, const double *totmassnuclide, const int k,
                      const int64_t i) {
  if (k < NCELLSUMS) return E.raw[k][i * E.est_stride] / nprocs;
  return vectors[(int64_t)(k - NCELLSUMS) * T.nnuclides + i] * totmassnuclide[i];
}

// sn3d.cc:247-250: cell c's term of totmassnuclide[nuc] (nuc < 0: of mtot)
AHD double totmass_term(const float *rho_tmin, const double *assocvolume_tmin, const float *X, const int64_t stride, const int64_t c, const int nuc) {
  const double cellmass = rho_tmin[c] * assocvolume_tmin[c];
  return nuc < 0 ? cellmass : cellmass * X[(int64_t)nuc * stride + c];
}

// ---- host: validation and the row structure (plain C++)

struct Rows {
  std::vector<double> energy;  // [NVECTORS][nnuclides]
  std::vector<int32_t> top_start, top_path, top_end, rad_nuc;
};

// empty: the model is usable with a decay set-up of nnuclides nuclides on ncell cells; else what is wrong with it, naming the nuclide
inline std::string deposition_validate(const artis_deposition_model &m, const int nnuclides, const int64_t ncell) {
  const auto finite_nonneg = [](double v) { return std::isfinite(v) && v >= 0.; };
  if (m.nnuclides != nnuclides) return "nnuclides is not the decay set-up's (" + std::to_string(nnuclides) + ")";
  if (m.npts_nonempty != ncell) return "npts_nonempty is not the decay set-up's (" + std::to_string(ncell) + ")";
  if (nnuclides > 0 && (!m.nuc_endecay_gamma || !m.nuc_endecay_particle || !m.nuc_endecay_q || !m.nuc_branchprob))
    return "nuc_endecay_gamma, nuc_endecay_particle, nuc_endecay_q and nuc_branchprob are required";
  if (ncell > 0 && (!m.assocvolume_tmin || !m.radial_pos_tmin)) return "assocvolume_tmin and radial_pos_tmin are required";
  for (int n = 0; n < nnuclides; n++) {
    const std::string name = "nuclide " + std::to_string(n) + ": ";
    if (!finite_nonneg(m.nuc_endecay_gamma[n])) return name + "a negative or non-finite endecay_gamma";
    for (int t = 0; t < NQDOT; t++) {
      if (!finite_nonneg(m.nuc_endecay_particle[n * NQDOT + t])) return name + "a negative or non-finite endecay_particle";
      if (!finite_nonneg(m.nuc_endecay_q[n * NQDOT + t])) return name + "a negative or non-finite endecay_q";
      const double b = m.nuc_branchprob[n * NQDOT + t];
      if (!(b >= 0. && b <= 1.)) return name + "a branch probability outside [0, 1]";
    }
  }
  for (int64_t c = 0; c < ncell; c++) {
    if (!(m.assocvolume_tmin[c] > 0.) || !std::isfinite(m.assocvolume_tmin[c])) return "cell " + std::to_string(c) + ": a non-positive or non-finite assocvolume_tmin";
    if (!finite_nonneg(m.radial_pos_tmin[c])) return "cell " + std::to_string(c) + ": a negative or non-finite radial_pos_tmin";
  }
  return "";
}

// of a validated model on a validated network: path_top, path_end [npaths] the paths' first and last nuclides, nuc_meanlife [nnuclides].
// *bad: empty, or what is wrong with the network (a path whose top is stable or out of range)
inline Rows build_dep_rows(const artis_deposition_model &m, const int nnuclides, const int npaths, const int32_t *path_top, const int32_t *path_end,
                           const double *nuc_meanlife, std::string *bad) {
  Rows r;
  bad->clear();
  const size_t nn = (size_t)nnuclides;
  r.energy.assign((size_t)NVECTORS * nn, 0.);
  static const int particle_type[NCHANNELS] = {-1, ARTIS_DECAYTYPE_BETAPLUS, ARTIS_DECAYTYPE_BETAMINUS, ARTIS_DECAYTYPE_ALPHA, ARTIS_DECAYTYPE_SPONTFISSION};
  for (size_t n = 0; n < nn; n++) {
    r.energy[n] = m.nuc_endecay_gamma[n];
    for (int ch = 1; ch < NCHANNELS; ch++)
      r.energy[(size_t)ch * nn + n] = m.nuc_endecay_particle[n * NQDOT + (size_t)particle_type[ch]] * m.nuc_branchprob[n * NQDOT + (size_t)particle_type[ch]];
    for (int t = 0; t < NQDOT; t++) r.energy[(size_t)(NCHANNELS + t) * nn + n] = m.nuc_endecay_q[n * NQDOT + (size_t)t] * m.nuc_branchprob[n * NQDOT + (size_t)t];
    if (nuc_meanlife[n] > 0.) r.rad_nuc.push_back((int32_t)n);
  }
  std::vector<std::vector<int32_t>> rows(nn);
  for (int p = 0; p < npaths; p++) {
    const int top = path_top[p], end = path_end[p];
    if (top < 0 || top >= nnuclides || end < 0 || end >= nnuclides) {
      *bad = "path " + std::to_string(p) + ": a nuclide index out of range";
      return r;
    }
    if (!(nuc_meanlife[top] > 0.)) {
      *bad = "path " + std::to_string(p) + ": its top nuclide " + std::to_string(top) + " is stable";
      return r;
    }
    rows[(size_t)top].push_back(p);
  }
  r.top_start.assign(nn + 1, 0);
  for (size_t n = 0; n < nn; n++) {
    r.top_start[n + 1] = r.top_start[n] + (int32_t)rows[n].size();
    for (int32_t p : rows[n]) {
      r.top_path.push_back(p);
      r.top_end.push_back(path_end[p]);
    }
  }
  return r;
}

// handed-in vectors [NVECTORS][nnuclides] are usable as they are: finite, non-negative, and +0 for every stable nuclide (the walk skips those)
inline std::string vectors_validate(const double *vectors, const int nnuclides, const double *nuc_meanlife) {
  for (int v = 0; v < NVECTORS; v++)
    for (int n = 0; n < nnuclides; n++) {
      const double p = vectors[(int64_t)v * nnuclides + n];
      if (!std::isfinite(p) || p < 0.) return "nuclide " + std::to_string(n) + ": a negative or non-finite power";
      if (!(nuc_meanlife[n] > 0.) && p != 0.) return "nuclide " + std::to_string(n) + ": a power for a stable nuclide";
    }
  return "";
}

// the view of host arrays and their rows
inline Tables host_tables(const Rows &r, const int nnuclides, const int npaths, const double *nuc_meanlife, const double *nuc_mass) {
  Tables T{};
  T.nnuclides = nnuclides;
  T.npaths = npaths;
  T.nrad = (int32_t)r.rad_nuc.size();
  T.nuc_meanlife = nuc_meanlife;
  T.nuc_mass = nuc_mass;
  T.energy = r.energy.data();
  T.top_start = r.top_start.data();
  T.top_path = r.top_path.data();
  T.top_end = r.top_end.data();
  T.rad_nuc = r.rad_nuc.data();
  return T;
}

}  // namespace artis_dep
