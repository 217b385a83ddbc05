// spectra.h -- per-packet rules of the emergent spectra and light curves.
//
// The reference bins its escaped packets after every timestep (write_partial_lightcurve_spectra, sn3d.cc:806) and at the
// end (exspec.cc:30-130) with add_to_spec_res / add_to_lc_res (spectrum_lightcurve.cc:544-713). The functions here are
// what one packet contributes there: which output element it adds to and how much. The engine's kernels
// (artis_engine.hip, "spectra") sum the contributions of every output element sequentially in the caller's packet
// order; tests/spectra_host compiles the same functions for x86 and sums them in a plain loop.
//
// Floating-point discipline as physics.h: -ffp-contract=off, and every expression keeps the reference's order of
// operations. nprocs_exspec is 1 (a division by 1 is exact, so it is left out).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/artis_amd.h"

#if defined(__HIPCC__) && !defined(ARTIS_HOST_EMU)
#define SPEC_AHD __host__ __device__ inline
#else
#define SPEC_AHD inline
#endif

namespace artis_spec {

constexpr double CLIGHT = 2.99792458e+10;  // constants.h
constexpr double PI = 3.14159265358979323846;
constexpr double PARSEC = 3.0857e+18;     // constants.h:39
constexpr double MEV = 1.6021772e-6;
constexpr double H = 6.6260755e-27;
constexpr int MNUBINS = 1000;             // exspec.h:8
constexpr int NPHIBINS = 10, NCOSTHETABINS = 10;  // exspec.h:10-11
constexpr int MABINS = NPHIBINS * NCOSTHETABINS;  // exspec.h:12
constexpr double NU_MIN_GAMMA = 0.05 * MEV / H;   // exspec.cc:61
constexpr double NU_MAX_GAMMA = 4. * MEV / H;     // exspec.cc:62
constexpr int TYPE_GAMMA = 10, TYPE_RPKT = 11, TYPE_ESCAPE = 32;

// get_escapedirectionbin (vectors.h:147): costheta bin about syn_dir = z (constants.h:94) times NPHIBINS plus the phi bin,
// the phi bins in decreasing phi order
SPEC_AHD int escapedirectionbin(const double dir_in[3]) {
  const double xhat[3] = {1.0, 0.0, 0.0};
  const double syn[3] = {0.0, 0.0, 1.0};
  const double dirmag = sqrt(dir_in[0] * dir_in[0] + dir_in[1] * dir_in[1] + dir_in[2] * dir_in[2]);
  const double dir[3] = {dir_in[0] / dirmag, dir_in[1] / dirmag, dir_in[2] / dirmag};
  const double costheta = dir[0] * syn[0] + dir[1] * syn[1] + dir[2] * syn[2];
  int costhetabin = (int)((costheta + 1.0) * NCOSTHETABINS / 2.0);
  costhetabin = costhetabin < 0 ? 0 : (costhetabin > NCOSTHETABINS - 1 ? NCOSTHETABINS - 1 : costhetabin);
  // cross_prod(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)
  const double vec1[3] = {dir[1] * syn[2] - dir[2] * syn[1], dir[2] * syn[0] - dir[0] * syn[2], dir[0] * syn[1] - dir[1] * syn[0]};
  const double vec2[3] = {xhat[1] * syn[2] - xhat[2] * syn[1], xhat[2] * syn[0] - xhat[0] * syn[2], xhat[0] * syn[1] - xhat[1] * syn[0]};
  const double vec1_len = sqrt(vec1[0] * vec1[0] + vec1[1] * vec1[1] + vec1[2] * vec1[2]);
  double cosphi = 1.0;
  if (vec1_len > 1e-12) {
    cosphi = (vec1[0] * vec2[0] + vec1[1] * vec2[1] + vec1[2] * vec2[2]) / vec1_len;
    cosphi = cosphi < -1.0 ? -1.0 : (cosphi > 1.0 ? 1.0 : cosphi);
  }
  const double vec3[3] = {vec2[1] * syn[2] - vec2[2] * syn[1], vec2[2] * syn[0] - vec2[0] * syn[2], vec2[0] * syn[1] - vec2[1] * syn[0]};
  const double testphi = vec1[0] * vec3[0] + vec1[1] * vec3[1] + vec1[2] * vec3[2];
  const double phi = testphi > 0 ? acos(cosphi) : acos(cosphi) + PI;
  int phibin = (int)(phi / 2. / PI * NPHIBINS);
  phibin = phibin < 0 ? 0 : (phibin > NPHIBINS - 1 ? NPHIBINS - 1 : phibin);
  return costhetabin * NPHIBINS + phibin;
}

// A log-spaced frequency grid (init_spectra, spectrum_lightcurve.cc:487): log(nu_min) and dlognu are formed once on the
// host; the edges are the reference's float32 lower_freq / delta_freq.
struct SpecGrid {
  double nu_min, nu_max, log_nu_min, dlognu;
  const float *delta_freq;  // [MNUBINS]
};

// init_spectra (:487-504) with get_loggrid_edge (sn3d.h:142); on the host, once per grid
inline SpecGrid make_grid(double nu_min, double nu_max, float *lower_freq, float *delta_freq) {
  SpecGrid g;
  g.nu_min = nu_min;
  g.nu_max = nu_max;
  g.dlognu = (log(nu_max) - log(nu_min)) / MNUBINS;
  g.log_nu_min = log(nu_min);
  for (int nnu = 0; nnu < MNUBINS; nnu++) {
    lower_freq[nnu] = (float)exp(log(nu_min) + ((double)nnu * g.dlognu));
    delta_freq[nnu] = (float)(exp(log(nu_min) + ((double)(nnu + 1) * g.dlognu)) - (double)lower_freq[nnu]);
  }
  g.delta_freq = delta_freq;
  return g;
}

// get_logbinindex (sn3d.h:134)
SPEC_AHD int logbinindex(double value, const SpecGrid &g) {
  const double x = floor((log(value) - g.log_nu_min) / g.dlognu);
  int64_t i = (int64_t)x;
  return (int)(i < 0 ? 0 : (i > MNUBINS - 1 ? MNUBINS - 1 : i));
}

// The time grid of the caller: timestep nts is [start[nts], start[nts + 1]), the last one ends at tmax.
struct SpecTimes {
  int32_t ntimesteps;
  const double *start, *width;
  double tmin, tmax;
};

// get_timestep (spectrum_lightcurve.cc:209) for a time that has passed tmin < t < tmax; -1 before the first start.
// The starts increase strictly (checked by the library), so a bisection finds the one timestep the reference's loop finds.
SPEC_AHD int timestep_of(double t, const SpecTimes &T) {
  if (!(t >= T.start[0])) return -1;
  int lo = 0, hi = T.ntimesteps;  // start[lo] <= t; the answer is in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (T.start[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// Column maps of the emission / absorption decomposition.
struct SpecColumns {
  int32_t nelements, max_nions, nlines, nbfcontinua;
  const int32_t *line_elementindex, *line_ionindex;  // [nlines]
  const int32_t *bf_col;                             // [nbfcontinua] element * max_nions + ion of bflist entry i, -1: none
};

SPEC_AHD int proccount(const SpecColumns &c) { return 2 * c.nelements * c.max_nions + 1; }  // get_proccount :166

// The bflist entries of one ion's levels (get_emtype_continuum, atomic.h:508: emission type -1 - (level_bflist_start + t)
// for photoionisation target t): bf_col[-1 - et] = element * max_nions + ion for every target of every ionising level. Entries that
// no target fills keep the caller's -1.
SPEC_AHD void fill_bf_columns_of_ion(int ui, const int32_t *ion_element, const int32_t *elem_uniqueionindexstart,
                                     const int32_t *ion_uniquelevelindexstart, const int32_t *ion_nlevels_ionising,
                                     const int32_t *level_nphixstargets, const int32_t *level_bflist_start, int max_nions,
                                     int nbfcontinua, int32_t *bf_col) {
  const int element = ion_element[ui];
  const int ion = ui - elem_uniqueionindexstart[element];
  const int l0 = ion_uniquelevelindexstart[ui];
  for (int level = 0; level < ion_nlevels_ionising[ui]; level++)
    for (int t = 0; t < level_nphixstargets[l0 + level]; t++) {
      const int bf = level_bflist_start[l0 + level] + t;
      if (bf >= 0 && bf < nbfcontinua) bf_col[bf] = element * max_nions + ion;
    }
}

// columnindex_from_emissiontype (spectrum_lightcurve.cc:168-203); -1: not counted (EMTYPE_NOTSET, or a type outside the model)
SPEC_AHD int emission_column(int et, const SpecColumns &c) {
  const int nemax = c.nelements * c.max_nions;
  if (et >= 0) {  // bound-bound
    if (et >= c.nlines) return -1;
    return c.line_elementindex[et] * c.max_nions + c.line_ionindex[et];
  }
  if (et == ARTIS_EMTYPE_FREEFREE) return 2 * nemax;
  if (et == ARTIS_EMTYPE_NOTSET) return -1;
  if (c.nbfcontinua == 0) return 2 * nemax;  // no bound-free continua: the free-free column (:190-193)
  const int bf = -1 - et;
  if (bf >= c.nbfcontinua || c.bf_col[bf] < 0) return -1;  // (bf_col -1: an entry that no level's target fills)
  return nemax + c.bf_col[bf];
}

// the absorption column of a bound-bound absorption (:615-626); -1 for every other absorption type
SPEC_AHD int absorption_column(int at, const SpecColumns &c) {
  if (at < 0 || at >= c.nlines) return -1;
  return c.line_elementindex[at] * c.max_nions + c.line_ionindex[at];
}

// What one packet contributes, whatever the outputs asked for. Bins are -1 where the packet does not count.
struct SpecPkt {
  int32_t kind;     // 0: not counted, 1: escaped r-packet, 2: escaped gamma packet
  int32_t dirbin;   // get_escapedirectionbin (r-packets)
  int32_t nts;      // timestep of the arrival time t_arrive (light curve)
  int32_t ntc;      // timestep of the comoving escape time (comoving light curve)
  int32_t nnu;      // frequency bin (r-packet grid, or the gamma grid for a gamma packet); -1 unless nts >= 0 and nu in range
  int32_t nnu_abs;  // bin of the absorption frequency, -1 unless nnu >= 0, a bound-bound absorption and the frequency in range
  int32_t emcol, truecol, abscol;  // columns (-1: none)
  int32_t pad;
  double e_rf, e_cmf, stokes_q, stokes_u;
};

struct SpecRules {
  SpecTimes T;
  SpecGrid r, g;       // r-packet and gamma frequency grids
  SpecColumns cols;
  double inverse_gamma;  // sqrt(1 - vmax^2/c^2) (:703)
  int32_t want_columns;  // classify the emission / absorption columns
};

// add_to_lc_res / add_to_spec_res (:544-713) up to the additions
SPEC_AHD SpecPkt classify(const artis_packet &p, const SpecRules &R) {
  SpecPkt s;
  s.kind = 0; s.dirbin = -1; s.nts = -1; s.ntc = -1; s.nnu = -1; s.nnu_abs = -1;
  s.emcol = -1; s.truecol = -1; s.abscol = -1; s.pad = 0;
  s.e_rf = p.e_rf; s.e_cmf = p.e_cmf; s.stokes_q = p.stokes_q; s.stokes_u = p.stokes_u;
  if (p.type != TYPE_ESCAPE) return s;
  if (p.escape_type == TYPE_RPKT) s.kind = 1;
  else if (p.escape_type == TYPE_GAMMA) s.kind = 2;
  else return s;
  if (s.kind == 1) s.dirbin = escapedirectionbin(p.dir);
  const double t_arrive = p.escape_time - ((p.pos[0] * p.dir[0] + p.pos[1] * p.dir[1] + p.pos[2] * p.dir[2]) / CLIGHT);  // :555
  if (t_arrive > R.T.tmin && t_arrive < R.T.tmax) s.nts = timestep_of(t_arrive, R.T);
  const double t_escape_cmf = p.escape_time * R.inverse_gamma;  // :705
  if (t_escape_cmf > R.T.tmin && t_escape_cmf < R.T.tmax) s.ntc = timestep_of(t_escape_cmf, R.T);
  const SpecGrid &G = s.kind == 1 ? R.r : R.g;
  if (s.nts >= 0 && p.nu_rf > G.nu_min && p.nu_rf < G.nu_max) s.nnu = logbinindex(p.nu_rf, G);
  if (s.kind == 1 && s.nnu >= 0 && R.want_columns) {
    s.truecol = emission_column(p.trueemissiontype, R.cols);
    s.emcol = emission_column(p.emissiontype, R.cols);
    s.abscol = absorption_column(p.absorptiontype, R.cols);
    if (s.abscol >= 0 && p.absorptionfreq > R.r.nu_min && p.absorptionfreq < R.r.nu_max) s.nnu_abs = logbinindex(p.absorptionfreq, R.r);
    else s.abscol = -1;
  }
  return s;
}

// light_curve_lum[nts] += (:698)
SPEC_AHD double lum_value(const SpecPkt &s, const SpecTimes &T, double solidanglefactor) {
  return s.e_rf / T.width[s.nts] * solidanglefactor;
}
// light_curve_lumcmf[nts] += (:710)
SPEC_AHD double lumcmf_value(const SpecPkt &s, const SpecTimes &T, double solidanglefactor, double inverse_gamma) {
  return s.e_cmf / T.width[s.ntc] * solidanglefactor / inverse_gamma;
}
// deltaE of a frequency bin (:563-564, :617-618)
SPEC_AHD double flux_value(double e_rf, double width, float delta_freq, double solidanglefactor) {
  return e_rf / width / (double)delta_freq / 4.e12 / PI / PARSEC / PARSEC * solidanglefactor;
}

// ---- output families: an output array, or the 2-3 arrays (I, Q, U) that share one slot per contribution
enum SpecFamily { FAM_LUM, FAM_LUMCMF, FAM_FLUX, FAM_EM, FAM_TRUEEM, FAM_ABS, FAM_GLUM, FAM_GLUMCMF, FAM_GFLUX, NFAM };
// outputs, in the order of the fields of artis_spectra (and of the device block)
enum SpecOutput { OUT_LUM, OUT_LUMCMF, OUT_FLUX, OUT_FLUX_Q, OUT_FLUX_U, OUT_EM, OUT_EM_Q, OUT_EM_U, OUT_TRUEEM, OUT_ABS, OUT_ABS_Q,
                  OUT_ABS_U, OUT_GLUM, OUT_GLUMCMF, OUT_GFLUX, NOUT };

struct SpecShape {
  int32_t dirbin;     // -1, 0..MABINS-1, or ARTIS_SPEC_ALL_DIRBINS
  int32_t ndirslots;  // 1, or 1 + MABINS
  int32_t ntimesteps, proccount, nabscols;
  int32_t emission_absorption, stokes, gamma;
};

SPEC_AHD bool family_on(int fam, const SpecShape &S) {
  if (fam == FAM_EM || fam == FAM_TRUEEM || fam == FAM_ABS) return S.emission_absorption != 0;
  if (fam >= FAM_GLUM) return S.gamma != 0;
  return true;
}
SPEC_AHD int family_ncomp(int fam, const SpecShape &S) {  // I, Q, U; trueemission has no Q / U (:569-596, :627-633)
  return ((fam == FAM_FLUX || fam == FAM_EM || fam == FAM_ABS) && S.stokes) ? 3 : 1;
}
SPEC_AHD int family_output(int fam, int comp) {
  switch (fam) {
    case FAM_LUM: return OUT_LUM;
    case FAM_LUMCMF: return OUT_LUMCMF;
    case FAM_FLUX: return OUT_FLUX + comp;
    case FAM_EM: return OUT_EM + comp;
    case FAM_TRUEEM: return OUT_TRUEEM;
    case FAM_ABS: return OUT_ABS + comp;
    case FAM_GLUM: return OUT_GLUM;
    case FAM_GLUMCMF: return OUT_GLUMCMF;
    default: return OUT_GFLUX;
  }
}
// elements of one direction slot of a family's arrays
SPEC_AHD int64_t family_slot_size(int fam, const SpecShape &S) {
  const int64_t T = S.ntimesteps, BT = (int64_t)MNUBINS * T;
  switch (fam) {
    case FAM_LUM: case FAM_LUMCMF: case FAM_GLUM: case FAM_GLUMCMF: return T;
    case FAM_FLUX: case FAM_GFLUX: return BT;
    case FAM_EM: case FAM_TRUEEM: return BT * S.proccount;
    default: return BT * S.nabscols;
  }
}
SPEC_AHD int64_t family_size(int fam, const SpecShape &S) {
  return family_slot_size(fam, S) * (fam >= FAM_GLUM ? 1 : S.ndirslots);
}
// Entries of a family: 2 per packet with all direction bins (entry e < n: the angle average of packet e; e >= n: the direction
// bin of packet e - n), one otherwise. *slot: the output element, *saf: the solidanglefactor (:562, :691). False: no contribution.
SPEC_AHD bool family_entry(int fam, const SpecShape &S, const SpecPkt &s, int half, int64_t *slot, double *saf) {
  const bool gamma_fam = fam >= FAM_GLUM;
  if (s.kind != (gamma_fam ? 2 : 1)) return false;
  int64_t d = 0;
  *saf = 1.;
  if (!gamma_fam) {
    if (S.dirbin == ARTIS_SPEC_ALL_DIRBINS) {
      if (half) {
        d = 1 + s.dirbin;
        *saf = MABINS;
      }
    } else if (S.dirbin >= 0) {
      if (s.dirbin != S.dirbin) return false;
      *saf = MABINS;
    }
  } else if (half) {
    return false;
  }
  const int64_t T = S.ntimesteps;
  int64_t k;
  switch (fam) {
    case FAM_LUM: case FAM_GLUM:
      if (s.nts < 0) return false;
      k = s.nts;
      break;
    case FAM_LUMCMF: case FAM_GLUMCMF:
      if (s.ntc < 0) return false;
      k = s.ntc;
      break;
    case FAM_FLUX: case FAM_GFLUX:
      if (s.nnu < 0) return false;
      k = s.nnu * T + s.nts;
      break;
    case FAM_EM:
      if (s.nnu < 0 || s.emcol < 0) return false;
      k = (s.nnu * T + s.nts) * S.proccount + s.emcol;
      break;
    case FAM_TRUEEM:
      if (s.nnu < 0 || s.truecol < 0) return false;
      k = (s.nnu * T + s.nts) * S.proccount + s.truecol;
      break;
    default:  // FAM_ABS
      if (s.nnu_abs < 0 || s.abscol < 0) return false;
      k = (s.nnu_abs * T + s.nts) * S.nabscols + s.abscol;
      break;
  }
  *slot = d * family_slot_size(fam, S) + k;
  return true;
}
// the contribution of an entry (comp 0: I, 1: Q, 2: U)
SPEC_AHD double family_value(int fam, int comp, const SpecPkt &s, const SpecRules &R, double saf) {
  double v;
  switch (fam) {
    case FAM_LUM: case FAM_GLUM: return lum_value(s, R.T, saf);
    case FAM_LUMCMF: case FAM_GLUMCMF: return lumcmf_value(s, R.T, saf, R.inverse_gamma);
    case FAM_GFLUX: return flux_value(s.e_rf, R.T.width[s.nts], R.g.delta_freq[s.nnu], saf);
    case FAM_ABS: v = flux_value(s.e_rf, R.T.width[s.nts], R.r.delta_freq[s.nnu_abs], saf); break;
    default: v = flux_value(s.e_rf, R.T.width[s.nts], R.r.delta_freq[s.nnu], saf); break;  // FLUX, EM, TRUEEM
  }
  return comp == 0 ? v : (comp == 1 ? s.stokes_q * v : s.stokes_u * v);
}

}  // namespace artis_spec
