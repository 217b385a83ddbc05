// initial_state_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The bodies of artis_amd/csrc/initial_state.h -- the ones the engine's kernels call -- compiled for x86 with g++ and applied in plain
// loops (cells split over a few std::threads) to host arrays: what artis_amd_initial_state computes on the device. Also exports the
// validator and the Bateman sum with the expansion factor, for tests/test_initial_state_rules.py. The elements' atomic numbers are an
// array of the call's own, so the lanthanide sum needs no special model.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/initial_state.h"

namespace {
struct HostInit {
  int64_t ncell;
  int nn, np;
  double tmin;
  std::vector<double> meanlife, mass, path_lambda, branch, endecay_gamma, endecay_particle, probsum, initq, radial;
  std::vector<int32_t> path_start, path_nuc, path_type, path_top;
  std::vector<float> X, rho_tmin;  // X [nuclide][cell], as the engine keeps it
  artis_pinit::Tables T;
};
std::string g_error;

template <class F>
void parallel_range(int64_t n, int nthreads, F work) {
  const int nt = nthreads > 1 ? nthreads : 1;
  std::vector<std::thread> pool;
  const int64_t chunk = (n + nt - 1) / nt;
  for (int t = 0; t < nt; t++) {
    const int64_t c0 = t * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;
    if (c0 < c1) pool.emplace_back(work, c0, c1);
  }
  for (auto &th : pool) th.join();
}

artis_init::Grey make_grey(const artis_initial_params *p, const int32_t *elem_anumber, int nelements) {
  artis_init::Grey G{};
  G.type = p->rpkt_grey_type;
  G.mfegroup = p->mfegroup;
  G.mtot_input = p->mtot_input;
  G.ffegrp = p->ffegrp;
  G.initelectronfrac = p->initelectronfrac;
  G.elem_anumber = elem_anumber;
  G.nelements = nelements;
  return G;
}

artis_dep::Step make_step(const artis_initial_params *p, double tmin, double rmax) {
  artis_dep::Step S{};
  S.t_mid = p->tstart;
  S.tmin = tmin;
  S.rmax = rmax;
  S.nts_next = p->nts_first;
  S.num_grey_timesteps = p->num_grey_timesteps;
  S.optical_depth_is_thick = p->optical_depth_is_thick;
  S.optical_depth_is_thick_vpkt = p->optical_depth_is_thick_vpkt;
  return S;
}
}  // namespace

extern "C" {

const char *init_host_last_error(void) { return g_error.c_str(); }
double init_host_mintemp(void) { return ARTIS_OPT_MINTEMP; }
double init_host_maxtemp(void) { return ARTIS_OPT_MAXTEMP; }
int init_host_depth(void) { return artis_pinit::CKPT_DEPTH; }

// out: {abund, scale, x_dom} of decaychain_expansion
void init_host_decaychain_expansion(const double *lambdas, int n, double timediff, double *out) {
  const artis_decay::Chain ch = artis_init::decaychain_expansion(lambdas, n, timediff);
  out[0] = ch.abund, out[1] = ch.scale, out[2] = ch.x_dom;
}

// initial_validate's text ("" for usable parameters)
const char *init_host_validate(const artis_initial_params *p, int64_t ncell, double t_model) {
  g_error = artis_init::initial_validate(*p, ncell, t_model);
  return g_error.c_str();
}

// the tables of validated models on ncell cells (nothing of them has to outlive the call); NULL with the text otherwise
void *init_host_new(const artis_decay_model *d, const artis_deposition_model *em, const artis_packet_init_model *m, int64_t ncell, double tmin) {
  g_error = artis_decay::decay_validate(*d, ncell, 0);
  if (g_error.empty()) g_error = artis_dep::deposition_validate(*em, d->nnuclides, ncell);
  bool unsupported = false;
  if (g_error.empty()) g_error = artis_pinit::packet_init_validate(*m, d->nnuclides, ncell, d->nuc_meanlife, tmin, d->t_model, &unsupported);
  if (!g_error.empty()) return nullptr;
  HostInit *h = new HostInit();
  h->ncell = ncell;
  h->tmin = tmin;
  const int nn = h->nn = d->nnuclides, np = h->np = d->npaths;
  h->meanlife.assign(d->nuc_meanlife, d->nuc_meanlife + nn);
  std::vector<double> lambda;
  for (int n = 0; n < nn; n++) {
    h->mass.push_back(d->nuc_a[n] * artis::MH);
    lambda.push_back(d->nuc_meanlife[n] > 0. ? 1. / d->nuc_meanlife[n] : 0.);
  }
  const int64_t nflat = np > 0 ? d->path_start[np] : 0;
  h->path_start.assign(d->path_start, d->path_start + np + 1);
  h->path_nuc.assign(d->path_nucindex, d->path_nucindex + nflat);
  h->path_type.assign(d->path_last_decaytype, d->path_last_decaytype + np);
  h->branch.assign(d->path_branchproduct, d->path_branchproduct + np);
  for (int64_t i = 0; i < nflat; i++) h->path_lambda.push_back(lambda[(size_t)d->path_nucindex[i]]);
  for (int p = 0; p < np; p++) h->path_top.push_back(d->path_nucindex[d->path_start[p]]);
  h->endecay_gamma.assign(em->nuc_endecay_gamma, em->nuc_endecay_gamma + nn);
  h->endecay_particle.assign(em->nuc_endecay_particle, em->nuc_endecay_particle + (int64_t)nn * artis_pinit::NDECAYTYPES);
  h->radial.assign(em->radial_pos_tmin, em->radial_pos_tmin + ncell);
  h->probsum.assign(m->nuc_decay_daughters_probsum, m->nuc_decay_daughters_probsum + nn);
  const bool channel = m->initial_packets_on && m->use_model_initial_energy;
  if (channel) h->initq.assign(m->initenergyq, m->initenergyq + ncell);
  h->rho_tmin.assign(d->rho_tmin, d->rho_tmin + ncell);
  h->X.resize((size_t)(ncell * nn));
  for (int64_t c = 0; c < ncell; c++)
    for (int n = 0; n < nn; n++) h->X[(size_t)(n * ncell + c)] = d->initnucmassfrac[c * nn + n];
  artis_pinit::Tables &T = h->T;
  T = artis_pinit::Tables{};
  T.nnuclides = nn;
  T.npaths = np;
  T.path_start = h->path_start.data();
  T.path_nucindex = h->path_nuc.data();
  T.path_last_decaytype = h->path_type.data();
  T.path_top = h->path_top.data();
  T.path_lambda = h->path_lambda.data();
  T.path_branchproduct = h->branch.data();
  T.nuc_meanlife = h->meanlife.data();
  T.nuc_mass = h->mass.data();
  T.endecay_gamma = h->endecay_gamma.data();
  T.endecay_particle = h->endecay_particle.data();
  T.probsum = h->probsum.data();
  T.initenergyq = channel ? h->initq.data() : nullptr;
  T.t_model = d->t_model;
  T.tmin = tmin;
  T.tmax = m->tmax;
  T.initial_packets_on = m->initial_packets_on ? 1 : 0;
  return h;
}
void init_host_free(void *h) { delete static_cast<HostInit *>(h); }

// the energy vector with the expansion factor, the chains' scale and x_dom [npaths]
void init_host_energy(const void *hv, double tstart, double *E, double *scale, double *x_dom) {
  const HostInit &h = *static_cast<const HostInit *>(hv);
  for (int p = 0; p < h.np; p++) E[p] = artis_init::path_energy_expansion(h.T, p, tstart, &scale[p], &x_dom[p]);
}

// Every cell with the vector E, rho [ncell] and massfrac [ncell][nelements] of the decay update at tstart: the arrays [ncell];
// counts {inside, below, above, non-finite, invalid kappagrey}; *first: the lowest non-finite cell, -1 without one
void init_host_cells(const void *hv, const artis_initial_params *p, const double *E, double rmax, const float *rho, const float *massfrac,
                     const int32_t *elem_anumber, int nelements, float *T_initial, double *endecay, float *kappagrey, float *grey_depth, int32_t *thick,
                     int32_t *flags, int64_t *counts, int32_t *first, int nthreads) {
  const HostInit &h = *static_cast<const HostInit *>(hv);
  const artis_init::CellIn in{h.rho_tmin.data(), rho, massfrac, h.T.initenergyq, h.radial.data(), h.tmin, p->tstart};
  const artis_init::Grey G = make_grey(p, elem_anumber, nelements);
  const artis_dep::Step S = make_step(p, h.tmin, rmax);
  const artis_init::CellOut out{T_initial, kappagrey, grey_depth, endecay, thick, flags};
  parallel_range(h.ncell, nthreads, [&](int64_t c0, int64_t c1) {
    for (int64_t c = c0; c < c1; c++) {
      const double sum = artis_pinit::cell_checkpoints(h.np, h.T.path_top, E, h.X.data(), h.ncell, c, nullptr, false);
      artis_init::cell_entry(sum, in, G, S, c, out);
    }
  });
  for (int k = 0; k < 5; k++) counts[k] = 0;
  *first = -1;
  for (int64_t c = 0; c < h.ncell; c++) {
    const int branch = flags[c] & ARTIS_INITIAL_BRANCH_MASK;
    counts[branch]++;
    if (flags[c] & ARTIS_INITIAL_KAPPA_INVALID) counts[4]++;
    if (branch == ARTIS_INITIAL_NONFINITE && *first < 0) *first = (int32_t)c;
  }
}

// kappagrey, grey depth and thickness of every cell from temperatures T_R given (the device's own T_initial)
void init_host_grey(const void *hv, const artis_initial_params *p, double rmax, const float *rho, const float *massfrac, const int32_t *elem_anumber,
                    int nelements, const float *T_R, float *kappagrey, float *grey_depth, int32_t *thick) {
  const HostInit &h = *static_cast<const HostInit *>(hv);
  const artis_init::Grey G = make_grey(p, elem_anumber, nelements);
  const artis_dep::Step S = make_step(p, h.tmin, rmax);
  for (int64_t c = 0; c < h.ncell; c++) {
    int32_t flag = 0;
    kappagrey[c] = artis_init::cell_kappagrey(G, c, h.rho_tmin[(size_t)c], T_R[c], massfrac + c * nelements, &flag);
    grey_depth[c] = artis_dep::cell_grey_depth(kappagrey[c], rho[c], h.radial[(size_t)c], S);
    thick[c] = artis_dep::cell_thickness(grey_depth[c], S);
  }
}

}  // extern "C"
