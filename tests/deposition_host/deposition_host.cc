// deposition_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The bodies of artis_amd/csrc/deposition.h -- the ones the engine's kernels call -- compiled for x86 with g++ and applied in plain
// loops (cells split over a few std::threads) to host arrays: what artis_amd_deposition_setup / _update compute on the device. Also
// exports the validator, the row builder and DEP_DEPTH for tests/test_deposition_rules.py. One library per options preset: the rules
// read PARTICLE_THERMALISATION_SCHEME and VPKT_ON.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/deposition.h"

namespace {
struct HostDep {
  int64_t ncell;
  int nn, np;
  std::vector<double> meanlife, mass, assocvol, radial;
  std::vector<float> X, rho_tmin;  // X [nuclide][cell], as the engine keeps it
  artis_dep::Rows rows;
  artis_dep::Tables T;
};
std::string g_error;

template <class F>
void parallel_cells(int64_t ncell, int nthreads, F work) {
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<std::thread> pool;
  const int64_t chunk = (ncell + nt - 1) / nt;
  for (int t = 0; t < nt; t++) {
    const int64_t c0 = t * chunk, c1 = c0 + chunk < ncell ? c0 + chunk : ncell;
    if (c0 < c1) pool.emplace_back(work, c0, c1);
  }
  for (auto &th : pool) th.join();
}

// step: {t_mid, tmin, rmax, prev_mid, prev_width, nprocs, nts_next, num_grey_timesteps, optical_depth_is_thick, optical_depth_is_thick_vpkt}
artis_dep::Step make_step(const double *s) {
  artis_dep::Step S{};
  S.t_mid = s[0], S.tmin = s[1], S.rmax = s[2], S.prev_mid = s[3], S.prev_width = s[4];
  S.nprocs = (int32_t)s[5], S.nts_next = (int32_t)s[6], S.num_grey_timesteps = (int32_t)s[7];
  S.optical_depth_is_thick = s[8], S.optical_depth_is_thick_vpkt = s[9];
  return S;
}
}  // namespace

extern "C" {

int dep_host_depth(void) { return artis_dep::DEP_DEPTH; }
int dep_host_instantfulldeposition(void) { return ARTIS_OPT_PARTICLE_THERMALISATION_SCHEME == ARTIS_PARTICLE_INSTANTFULLDEPOSITION; }
int dep_host_vpkt_on(void) { return ARTIS_OPT_VPKT_ON; }
const char *dep_host_last_error(void) { return g_error.c_str(); }

// deposition_validate's text ("" for a usable model)
const char *dep_host_validate(const artis_deposition_model *m, int nnuclides, int64_t ncell) {
  g_error = artis_dep::deposition_validate(*m, nnuclides, ncell);
  return g_error.c_str();
}

// the rows of a validated model over a validated network (nothing of either has to outlive the call); NULL with the text otherwise
void *dep_host_new(const artis_decay_model *d, const artis_deposition_model *m, int64_t ncell) {
  g_error = artis_decay::decay_validate(*d, ncell, 0);
  if (g_error.empty()) g_error = artis_dep::deposition_validate(*m, d->nnuclides, ncell);
  if (!g_error.empty()) return nullptr;
  HostDep *h = new HostDep();
  h->ncell = ncell;
  h->nn = d->nnuclides;
  h->np = d->npaths;
  std::vector<int32_t> top((size_t)h->np), end((size_t)h->np);
  for (int p = 0; p < h->np; p++) {
    top[(size_t)p] = d->path_nucindex[d->path_start[p]];
    end[(size_t)p] = d->path_nucindex[d->path_start[p + 1] - 1];
  }
  h->meanlife.assign(d->nuc_meanlife, d->nuc_meanlife + h->nn);
  for (int n = 0; n < h->nn; n++) h->mass.push_back(d->nuc_a[n] * artis::MH);
  h->rows = artis_dep::build_dep_rows(*m, h->nn, h->np, top.data(), end.data(), h->meanlife.data(), &g_error);
  if (!g_error.empty()) {
    delete h;
    return nullptr;
  }
  h->assocvol.assign(m->assocvolume_tmin, m->assocvolume_tmin + ncell);
  h->radial.assign(m->radial_pos_tmin, m->radial_pos_tmin + ncell);
  h->rho_tmin.assign(d->rho_tmin, d->rho_tmin + ncell);
  h->X.resize((size_t)(ncell * h->nn));
  for (int64_t c = 0; c < ncell; c++)
    for (int n = 0; n < h->nn; n++) h->X[(size_t)(n * ncell + c)] = d->initnucmassfrac[c * h->nn + n];
  h->T = artis_dep::host_tables(h->rows, h->nn, h->np, h->meanlife.data(), h->mass.data());
  return h;
}
void dep_host_free(void *h) { delete static_cast<HostDep *>(h); }

int dep_host_nrad(const void *h) { return static_cast<const HostDep *>(h)->T.nrad; }
// top_start [nnuclides + 1], top_path / top_end [npaths], rad_nuc [nrad]
void dep_host_rows(const void *hv, int32_t *top_start, int32_t *top_path, int32_t *top_end, int32_t *rad_nuc) {
  const artis_dep::Rows &r = static_cast<const HostDep *>(hv)->rows;
  const auto put = [](int32_t *to, const std::vector<int32_t> &v) {
    if (!v.empty()) std::memcpy(to, v.data(), sizeof(int32_t) * v.size());
  };
  put(top_start, r.top_start);
  put(top_path, r.top_path);
  put(top_end, r.top_end);
  put(rad_nuc, r.rad_nuc);
}

// the eleven power vectors [NVECTORS][nnuclides] from a timestep's coefficients
void dep_host_vectors(const void *hv, const double *endnuc_coeff, const double *survivingfrac, double *vectors) {
  const HostDep &h = *static_cast<const HostDep *>(hv);
  for (int v = 0; v < artis_dep::NVECTORS; v++)
    for (int n = 0; n < h.nn; n++) vectors[(int64_t)v * h.nn + n] = artis_dep::power_entry(h.T, endnuc_coeff, survivingfrac, v, n);
}

// "" or why handed-in vectors are refused
const char *dep_host_vectors_validate(const void *hv, const double *vectors) {
  const HostDep &h = *static_cast<const HostDep *>(hv);
  g_error = artis_dep::vectors_validate(vectors, h.nn, h.meanlife.data());
  return g_error.c_str();
}

// totmassnuclide [nnuclides] and mtot behind it
void dep_host_totmass(const void *hv, double *totmass) {
  const HostDep &h = *static_cast<const HostDep *>(hv);
  for (int b = 0; b <= h.nn; b++) {
    double s = 0.;
    for (int64_t c = 0; c < h.ncell; c++) s += artis_dep::totmass_term(h.rho_tmin.data(), h.assocvol.data(), h.X.data(), h.ncell, c, b < h.nn ? b : -1);
    totmass[b] = s;
  }
}

// The per-cell work of artis_amd_deposition_update: raw [4][ncell] {gamma, positron, electron, alpha}; eps_ana, dep [5][ncell].
// all_nuclides: the sums walk every nuclide from the vectors instead of the radioactive ones from their packed powers.
void dep_host_cells(const void *hv, const double *step, const double *vectors, const float *rho, const float *kappagrey, const double *raw,
                    double *eps_ana, double *dep, double *ntlepton, float *grey_depth, int32_t *thick, int all_nuclides, int nthreads) {
  const HostDep &h = *static_cast<const HostDep *>(hv);
  const artis_dep::Step S = make_step(step);
  const int nch = artis_dep::NCHANNELS;
  std::vector<double> pw((size_t)(nch * h.T.nrad) + 1);
  for (int k = 0; k < h.T.nrad; k++)
    for (int ch = 0; ch < nch; ch++) pw[(size_t)(k * nch + ch)] = vectors[(int64_t)ch * h.nn + h.T.rad_nuc[k]];
  artis_dep::Estimators E{};
  for (int k = 0; k < artis_dep::NCELLSUMS; k++) E.raw[k] = raw + k * h.ncell;
  E.est_stride = 1;
  const artis_dep::CellOut out{eps_ana, dep, ntlepton, grey_depth, thick};
  parallel_cells(h.ncell, nthreads, [&](int64_t c0, int64_t c1) {
    for (int64_t c = c0; c < c1; c++) {
      double sum[artis_dep::NCHANNELS];
      if (all_nuclides)
        artis_dep::cell_power_sums_all(h.T, vectors, h.X.data(), h.ncell, c, sum);
      else
        artis_dep::cell_power_sums(h.T, pw.data(), h.X.data(), h.ncell, c, sum);
      artis_dep::cell_entry(sum, S, E, rho, kappagrey, h.assocvol.data(), h.radial.data(), h.ncell, c, out);
    }
  });
}

// the fifteen totals
void dep_host_totals(const void *hv, int nprocs, const double *vectors, const double *raw, const double *totmass, double *totals) {
  const HostDep &h = *static_cast<const HostDep *>(hv);
  artis_dep::Estimators E{};
  for (int k = 0; k < artis_dep::NCELLSUMS; k++) E.raw[k] = raw + k * h.ncell;
  E.est_stride = 1;
  for (int k = 0; k < artis_dep::NTOTALS; k++) {
    double s = 0.;
    const int64_t n = artis_dep::total_length(h.T, h.ncell, k);
    for (int64_t i = 0; i < n; i++) s += artis_dep::total_term(h.T, E, nprocs, vectors, totmass, k, i);
    totals[k] = s;
  }
}

}  // extern "C"
