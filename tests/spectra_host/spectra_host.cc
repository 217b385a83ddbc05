// spectra_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The rules of artis_amd/csrc/spectra.h compiled for x86 with g++, summed the plain way: every output element adds its
// contributions one after the other in the caller's packet order, as exspec's loop does (exspec.cc:70-90). Compared
// bit for bit with the numpy restatements of tools/exspec.py; the engine's device binning must give the same arrays.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../artis_amd/csrc/spectra.h"

using namespace artis_spec;

namespace {
struct Host {
  std::vector<int32_t> bf_col;
  int max_nions = 0;
  SpecColumns cols{};
};
Host make_host(const artis_model *m, int nbf_override) {
  Host h;
  for (int el = 0; el < m->nelements; el++) h.max_nions = m->elem_nions[el] > h.max_nions ? m->elem_nions[el] : h.max_nions;
  h.bf_col.assign(m->nbfcontinua > 0 ? m->nbfcontinua : 1, -1);
  for (int ui = 0; ui < m->nions; ui++)
    fill_bf_columns_of_ion(ui, m->ion_element, m->elem_uniqueionindexstart, m->ion_uniquelevelindexstart, m->ion_nlevels_ionising,
                           m->level_nphixstargets, m->level_bflist_start, h.max_nions, m->nbfcontinua, h.bf_col.data());
  h.cols.nelements = m->nelements;
  h.cols.max_nions = h.max_nions;
  h.cols.nlines = m->nlines;
  h.cols.nbfcontinua = nbf_override >= 0 ? nbf_override : m->nbfcontinua;
  h.cols.line_elementindex = m->line_elementindex;
  h.cols.line_ionindex = m->line_ionindex;
  h.cols.bf_col = h.bf_col.data();
  return h;
}
}  // namespace

extern "C" {

// columnindex_from_emissiontype for one emission type (nbf_override >= 0: pretend the model has that many bf continua)
int spec_host_emission_column(const artis_model *m, int et, int nbf_override) {
  const Host h = make_host(m, nbf_override);
  return emission_column(et, h.cols);
}

// outs[NOUT]: the arrays of artis_spectra in field order (NULL: not produced), zero-filled by the caller;
// grids[4 * MNUBINS]: lower / delta of the r-packet grid, then of the gamma grid. Returns the escaped r-packets.
int64_t spec_host_compute(const artis_model *m, const artis_packet *pk, int64_t n, const artis_spectra_config *cfg, double nu_min_r,
                          double nu_max_r, int nbf_override, double **outs, float *grids) {
  const Host h = make_host(m, nbf_override);
  SpecRules R{};
  R.T.ntimesteps = cfg->ntimesteps;
  R.T.start = cfg->ts_start;
  R.T.width = cfg->ts_width;
  R.T.tmin = cfg->tmin;
  R.T.tmax = cfg->tmax;
  R.r = make_grid(nu_min_r, nu_max_r, grids, grids + MNUBINS);
  R.g = make_grid(NU_MIN_GAMMA, NU_MAX_GAMMA, grids + 2 * MNUBINS, grids + 3 * MNUBINS);
  R.cols = h.cols;
  R.inverse_gamma = sqrt(1. - (m->vmax * m->vmax / (CLIGHT * CLIGHT)));
  R.want_columns = cfg->emission_absorption != 0;
  SpecShape S{};
  S.dirbin = cfg->dirbin;
  S.ndirslots = cfg->dirbin == ARTIS_SPEC_ALL_DIRBINS ? 1 + MABINS : 1;
  S.ntimesteps = cfg->ntimesteps;
  S.nabscols = m->nelements * h.max_nions;
  S.proccount = 2 * S.nabscols + 1;
  S.emission_absorption = cfg->emission_absorption != 0;
  S.stokes = cfg->stokes != 0;
  S.gamma = cfg->gamma != 0;
  std::vector<SpecPkt> sp(n > 0 ? n : 1);
  int64_t nesc = 0;
  for (int64_t i = 0; i < n; i++) {
    sp[i] = classify(pk[i], R);
    nesc += sp[i].kind == 1;
  }
  const int64_t nent = n * (S.ndirslots > 1 ? 2 : 1);
  for (int fam = 0; fam < NFAM; fam++) {
    if (!family_on(fam, S)) continue;
    for (int64_t e = 0; e < nent; e++) {
      const int half = e >= n;
      int64_t slot;
      double saf;
      if (!family_entry(fam, S, sp[half ? e - n : e], half, &slot, &saf)) continue;
      for (int c = 0; c < family_ncomp(fam, S); c++) {
        double *o = outs[family_output(fam, c)];
        if (o) o[slot] += family_value(fam, c, sp[half ? e - n : e], R, saf);
      }
    }
  }
  return nesc;
}

}  // extern "C"
