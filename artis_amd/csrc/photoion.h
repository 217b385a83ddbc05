// photoion.h -- the photoionisation coefficients of builds without USE_LUT_PHOTOION: get_corrphotoioncoeff (ratecoeff.cc:840-868, the
// branch without the table) for every bound-free pair of a cell, with calculate_corrphotoioncoeff_integral (ratecoeff.cc:480-521), its
// integrand (ratecoeff.cc:463-478) and radfield::radfield (radfield.cc:786) on the adaptive 61-point Gauss-Kronrod integrator of
// bf_heating.h. The reference evaluates a coefficient when a packet first needs it in a cell; here every pair of every cell is made.
//
// The engine's kernel (stage_photoion.h) and the loops of tests/photoion_host (x86) call the same functions. Floating-point discipline
// as bf_heating.h and ratecoeff_tables.h: -ffp-contract=off, every expression in the reference's order of operations and float/double
// mixing; the integrand is templated on a Math policy: the stage's own exp and expm1 (artis_bfh::TbMath: a lane and the x86 build form
// the same bits) or libm's (the reference's arithmetic; the x86 harness builds both).
//
// Tepow[cell] = std::pow(T_e, -1.5) is made on the HOST with the host's libm (make_tepow) and handed in: the device's pow does not enter.
//
// WHAT IS NOT FINITE. modified_departure_ratio is 1 for a lower population that is not > 0 (a NaN among them) and 0 when it is not
// finite, so no population can make a coefficient non-finite; a T_e or a bin's T_R that is NaN can, and so can a NaN handed in as an
// estimator (NaN < 0 is false: it is taken). Such a coefficient is counted and sets the cell's flag (the reference's assert_always).
#pragma once
#include <vector>

#include "ratecoeff_tables.h"

namespace artis_pi {

using artis::DevModel;
using artis_bfh::Gk61Stats;
using artis_bfh::TbMath;
using artis_rc::PhixsGrid;

constexpr int NBINS = ARTIS_OPT_RADFIELDBINCOUNT;
constexpr double EPSREL = 1e-3;  // ratecoeff.cc:482
constexpr double FOURPI = 4 * artis::PI;
// which rule made an entry (0: no continuum of the model writes it)
constexpr uint8_t SRC_NONE = 0, SRC_ESTIMATOR = 1, SRC_INTEGRAL = 2;
constexpr int32_t NONFINITE = ARTIS_PHOTOION_NONFINITE;  // per-cell flag bit
constexpr int NTOTALS = ARTIS_PHOTOION_NTOTALS;  // entries from estimators, integrals, 61-point nodes, integrals at depth 15, non-finite coefficients

// the totals of one lane (or one x86 loop): integers, so that their sums do not depend on the order
struct Totals {
  int64_t v[NTOTALS];
  AHD void add(const Gk61Stats &s) {
    v[1] += 1;
    v[2] += s.nodes;
    v[3] += s.maxdepth >= (int32_t)artis_bfh::MAX_DEPTH;
  }
};

// one bin of the cell's multibin radiation field
struct BinWT {
  float W, T_R;
};

// radfield::radfield radfield.cc:786 of one cell, with radfield::planck (radfield.h:50) on the policy's expm1. bins: the cell's NBINS
// pairs (builds with MULTIBIN_RADFIELD_MODEL_ON, used when binned is set: nts >= FIRST_NLTE_RADFIELD_TIMESTEP); the kernel points it at LDS.
template <class Math>
struct CellRadfield {
  const BinWT *bins;
  int32_t binned;
  float W, T_R;  // the full-spectrum dilute black body
  static AHD double planck(const double nu, const double T) {
    return 2 * artis::HPLANCK * artis::pow3(nu) / artis::pow2(artis::CLIGHT) / Math::expm1(artis::HOVERKB * nu / T);
  }
  AHD double operator()(const double nu) const {
#if ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON
    if (binned) {
      const int b = artis::radbin_select(nu);
      if (b >= 0) {
        const BinWT bin = bins[b];
        if (bin.W >= 0.) return bin.W * planck(nu, bin.T_R);
      }
      return 0.;
    }
#endif
    return W * planck(nu, T_R);
  }
};

// integrand_corrphotoioncoeff_custom_radfield ratecoeff.cc:463, over nu_minus_nu_edge; the cross-section grid by value
template <class Math>
struct PiIntegrand {
  PhixsGrid g;
  double nu_edge, modified_departure_ratio;
  float T_e;
  CellRadfield<Math> J;
  AHD double operator()(const double nu_minus_nu_edge) const {
    double corrfactor = 1. - (modified_departure_ratio * Math::exp(-artis::HOVERKB * nu_minus_nu_edge / T_e));
    if (corrfactor < 0) corrfactor = 0.;
    const float sigma_bf = g.at(nu_edge, nu_minus_nu_edge + nu_edge);
    const double Jnu = J(nu_minus_nu_edge + nu_edge);
    return (1. / artis::HPLANCK) * sigma_bf / (nu_minus_nu_edge + nu_edge) * Jnu * corrfactor;
  }
};

// what a cell's entries share
struct CellIn {
  float T_e, clumpednne;  // grid::get_nne * grid::get_clumpfactor (floats: a float product)
  double Tepow;           // std::pow(T_e, -1.5), the host's
  const double *levelpops;  // the cell's row [nlevels]
};

// modified_departure_ratio ratecoeff.cc:497-505
AHD double departure_ratio(const DevModel &M, const int ul, const int ul_upper, const CellIn &c) {
  const double nnlevel = c.levelpops[ul];
  const double modified_sahafact = artis::SAHACONST * artis::statw(M, ul) / artis::statw(M, ul_upper) * c.Tepow;
  const double nnupperionlevel = c.levelpops[ul_upper];
  double modified_departure_ratio = nnlevel > 0. ? nnupperionlevel / nnlevel * c.clumpednne * modified_sahafact : 1.;
  if (!isfinite(modified_departure_ratio)) modified_departure_ratio = 0.;
  return modified_departure_ratio;
}

// calculate_corrphotoioncoeff_integral ratecoeff.cc:480 of target t of level ul
template <class Math>
AHD double pi_integral(const DevModel &M, const int ul, const int t, const CellIn &c, const CellRadfield<Math> &J, Totals *tot) {
  const int ui = M.level_ion[ul];
  const int element = M.ion_element[ui];
  const int ion = ui - M.elem_uniqueionindexstart[element];
  const int level = ul - M.ion_uniquelevelindexstart[ui];
  const double nu_threshold = (1. / artis::HPLANCK) * artis::phixs_threshold(M, element, ion, level, t);
  const double nu_max_phixs = nu_threshold * M.last_phixs_nuovernuedge;
  const int ul_upper = artis::lstart(M, element, ion + 1) + artis::phixs_upperlevel(M, ul, t);
  const double ratio = departure_ratio(M, ul, ul_upper, c);
  const PiIntegrand<Math> f{PhixsGrid{(int32_t)M.NPHIXSPOINTS, M.NPHIXSNUINCREMENT, M.last_phixs_nuovernuedge, artis::phixs_table(M, ul)}, nu_threshold, ratio,
                            c.T_e, J};
  double error = 0.;
  Gk61Stats st;
  const double integral = artis_bfh::gk61_integrate(f, 0, nu_max_phixs - nu_threshold, EPSREL, &error, &st);
  tot->add(st);
  return FOURPI * artis::phixs_probability(M, ul, t) * integral;
}

// ---- the arrays of a call: what the kernel (device pointers) and the x86 loops (host pointers) hand to the body below
struct Arrays {
  int64_t ncell;
  int32_t ncont;     // nbfcontinua: the continua of the allcont_* arrays
  int32_t nentries;  // nphixstargets_total
  int32_t nbfestim;
  int32_t use_bf_estimators;  // globals::timestep >= DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP, the host's statement
  int32_t binned;             // MULTIBIN_RADFIELD_MODEL_ON && nts >= FIRST_NLTE_RADFIELD_TIMESTEP
  const float *Te, *nne, *clumpfactor, *TR, *W;
  const double *Tepow;      // [ncell]
  const double *levelpops;  // [ncell][nlevels]
  const float *bin_W, *bin_T_R;  // [ncell][NBINS] (multibin builds)
  const float *bfrate_normed;    // [ncell][nbfestim] prev_bfrate_normed (used with use_bf_estimators)
  double *coeff;    // [ncell][nentries]
  uint8_t *source;  // [ncell][nentries]
  int32_t *flags;   // [ncell]
};

AHD CellIn cell_in(const DevModel &M, const Arrays &a, const int64_t c) {
  return CellIn{a.Te[c], a.nne[c] * a.clumpfactor[c], a.Tepow[c], a.levelpops + c * M.nlevels};
}
template <class Math>
AHD CellRadfield<Math> cell_radfield(const Arrays &a, const int64_t c, const BinWT *bins) {
  return CellRadfield<Math>{bins, a.binned, a.W[c], a.TR[c]};
}
// the cell's bins as pairs, where `to` lies (the kernel: LDS; x86: a local array)
AHD void stage_bin(const Arrays &a, const int64_t c, const int b, BinWT *to) {
  to[b] = BinWT{a.bin_W[c * NBINS + b], a.bin_T_R[c * NBINS + b]};
}

// get_corrphotoioncoeff ratecoeff.cc:847-868 of continuum i of the allcont_* arrays in cell c: entry level_phixstargetstart[ul] + t.
// Returns the bits for the cell's flags. Every entry has this one writer.
template <class Math>
AHD int32_t cont_cell_entry(const DevModel &M, const Arrays &a, const int64_t c, const int i, const CellIn &cell, const CellRadfield<Math> &J, Totals *tot) {
  const int ul = M.allcont_uniquelevelindex[i];
  const int t = M.allcont_phixstargetindex[i];
  const int64_t at = c * a.nentries + M.level_phixstargetstart[ul] + t;
  double gammacorr = -1;
  uint8_t source = SRC_INTEGRAL;
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
  if (a.use_bf_estimators) {
    const int bi = artis::bfestimindex(M, i);
    if (bi >= 0) gammacorr = a.bfrate_normed[c * a.nbfestim + bi];  // radfield::get_bfrate_estimator; -1 where there is no estimator
  }
#endif
  if (gammacorr < 0) {
    gammacorr = pi_integral<Math>(M, ul, t, cell, J, tot);
  } else {
    source = SRC_ESTIMATOR;
    tot->v[0] += 1;
  }
  a.coeff[at] = gammacorr;
  a.source[at] = source;
  if (isfinite(gammacorr)) return 0;
  tot->v[4] += 1;
  return NONFINITE;
}

// ---------------------------------------------------------------- host side
// Tepow[c] = std::pow(T_e, -1.5) (ratecoeff.cc:498: T_e is a float), with the host's libm
inline void make_tepow(const float *Te, const int64_t ncell, double *Tepow) {
  for (int64_t c = 0; c < ncell; c++) Tepow[c] = std::pow(Te[c], -1.5);
}

}  // namespace artis_pi
