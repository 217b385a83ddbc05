// packet_init_host.cc -- TEST HARNESS ONLY (never shipped, never loaded by the artis_amd package).
//
// The bodies of artis_amd/csrc/packet_init.h -- the ones the engine's kernels call -- compiled for x86 with g++ and applied in plain
// loops (packets and cells split over a few std::threads) to host arrays: what artis_amd_packet_init_setup / _packet_init compute on the
// device. Also exports the validator, lerp_std beside std::lerp, and the channel search by checkpoints beside the reference's whole
// running sum, for tests/test_packet_init_rules.py. C++20 for std::lerp.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../artis_amd/csrc/packet_init.h"

namespace {
struct HostPinit {
  int64_t ncell;
  int nn, np;
  std::vector<double> meanlife, mass, lambda, path_lambda, branch, endecay_gamma, endecay_particle, probsum, gamma_energy, gamma_prob, initq, coord[3];
  std::vector<int32_t> path_start, path_nuc, path_type, path_top, gamma_start, propcell;
  std::vector<float> X, rho_tmin;  // X [nuclide][cell], as the engine keeps it
  artis_pinit::Tables T;
  artis_pinit::Grid G;
  // of the last cells()
  std::vector<double> E, ckpt, endecay, en_cumulative;
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

artis_pinit::Work make_work(const HostPinit &h, double e_cmf_per_packet) {
  artis_pinit::Work W{};
  W.T = h.T;
  W.G = h.G;
  W.E = h.E.data();
  W.X = h.X.data();
  W.ncell = h.ncell;
  W.ckpt = h.ckpt.data();
  W.en_cumulative = h.en_cumulative.data();
  W.e_cmf_per_packet = e_cmf_per_packet;
  return W;
}
}  // namespace

extern "C" {

int pinit_host_stride(void) { return artis_pinit::CKPT_STRIDE; }
int pinit_host_default_trials(void) { return artis_pinit::DEFAULT_TRIALS_PER_LAUNCH; }
const char *pinit_host_last_error(void) { return g_error.c_str(); }
double pinit_host_lerp(double a, double b, double t) { return artis_pinit::lerp_std(a, b, t); }
double pinit_host_std_lerp(double a, double b, double t) { return std::lerp(a, b, t); }

// packet_init_validate's text ("" for a usable model); *unsupported as the set-up's return code tells it
const char *pinit_host_validate(const artis_packet_init_model *m, int nnuclides, int64_t ncell, const double *nuc_meanlife, double tmin, double t_model, int *unsupported) {
  bool u = false;
  g_error = artis_pinit::packet_init_validate(*m, nnuclides, ncell, nuc_meanlife, tmin, t_model, &u);
  *unsupported = u ? 1 : 0;
  return g_error.c_str();
}
const char *pinit_host_vector_validate(const double *E, int npaths) {
  g_error = artis_pinit::energy_vector_validate(E, npaths);
  return g_error.c_str();
}

// the tables of validated models on the grid of `model` (nothing of them has to outlive the call); NULL with the text otherwise
void *pinit_host_new(const artis_model *model, const artis_decay_model *d, const artis_deposition_model *em, const artis_packet_init_model *m) {
  const int64_t ncell = model->npts_nonempty;
  g_error = artis_decay::decay_validate(*d, ncell, 0);
  if (g_error.empty()) g_error = artis_dep::deposition_validate(*em, d->nnuclides, ncell);
  bool unsupported = false;
  if (g_error.empty()) g_error = artis_pinit::packet_init_validate(*m, d->nnuclides, ncell, d->nuc_meanlife, model->tmin, d->t_model, &unsupported);
  if (!g_error.empty()) return nullptr;
  HostPinit *h = new HostPinit();
  h->ncell = ncell;
  const int nn = h->nn = d->nnuclides, np = h->np = d->npaths;
  h->meanlife.assign(d->nuc_meanlife, d->nuc_meanlife + nn);
  for (int n = 0; n < nn; n++) {
    h->mass.push_back(d->nuc_a[n] * artis::MH);
    h->lambda.push_back(d->nuc_meanlife[n] > 0. ? 1. / d->nuc_meanlife[n] : 0.);
  }
  const int64_t nflat = np > 0 ? d->path_start[np] : 0;
  h->path_start.assign(d->path_start, d->path_start + np + 1);
  h->path_nuc.assign(d->path_nucindex, d->path_nucindex + nflat);
  h->path_type.assign(d->path_last_decaytype, d->path_last_decaytype + np);
  h->branch.assign(d->path_branchproduct, d->path_branchproduct + np);
  for (int64_t i = 0; i < nflat; i++) h->path_lambda.push_back(h->lambda[(size_t)d->path_nucindex[i]]);
  for (int p = 0; p < np; p++) h->path_top.push_back(d->path_nucindex[d->path_start[p]]);
  h->endecay_gamma.assign(em->nuc_endecay_gamma, em->nuc_endecay_gamma + nn);
  h->endecay_particle.assign(em->nuc_endecay_particle, em->nuc_endecay_particle + (int64_t)nn * artis_pinit::NDECAYTYPES);
  h->probsum.assign(m->nuc_decay_daughters_probsum, m->nuc_decay_daughters_probsum + nn);
  h->gamma_start.assign(m->gamma_start, m->gamma_start + nn + 1);
  const int nlines = h->gamma_start[(size_t)nn];
  if (nlines > 0) {
    h->gamma_energy.assign(m->gamma_energy, m->gamma_energy + nlines);
    h->gamma_prob.assign(m->gamma_probability, m->gamma_probability + nlines);
  }
  const bool channel = m->initial_packets_on && m->use_model_initial_energy;
  if (channel) h->initq.assign(m->initenergyq, m->initenergyq + ncell);
  h->rho_tmin.assign(d->rho_tmin, d->rho_tmin + ncell);
  h->X.resize((size_t)(ncell * nn));
  for (int64_t c = 0; c < ncell; c++)
    for (int n = 0; n < nn; n++) h->X[(size_t)(n * ncell + c)] = d->initnucmassfrac[c * nn + n];
  h->propcell.assign(model->propcell_nonemptymgi, model->propcell_nonemptymgi + model->ngrid);
  artis_pinit::Grid &G = h->G;
  G.gridtype = model->gridtype;
  G.ngrid = model->ngrid;
  int stride = 1;
  for (int a = 0; a < 3; a++) {
    G.ncoordgrid[a] = model->ncoordgrid[a];
    G.coordstride[a] = stride;
    stride *= model->ncoordgrid[a];
    if (model->coord_pos_min_tmin[a] && model->ncoordgrid[a] > 0) h->coord[a].assign(model->coord_pos_min_tmin[a], model->coord_pos_min_tmin[a] + model->ncoordgrid[a]);
    G.coord_pos_min_tmin[a] = h->coord[a].data();
  }
  G.propcell_nonemptymgi = h->propcell.data();
  G.rmax = model->rmax;
  G.tmin = model->tmin;
  artis_pinit::Tables &T = h->T;
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
  T.gamma_start = h->gamma_start.data();
  T.gamma_energy = h->gamma_energy.data();
  T.gamma_probability = h->gamma_prob.data();
  T.initenergyq = channel ? h->initq.data() : nullptr;
  T.t_model = d->t_model;
  T.tmin = model->tmin;
  T.tmax = m->tmax;
  T.initial_packets_on = m->initial_packets_on ? 1 : 0;
  return h;
}
void pinit_host_free(void *h) { delete static_cast<HostPinit *>(h); }

// the energy vector [npaths]
void pinit_host_energy(const void *hv, double *E) {
  const HostPinit &h = *static_cast<const HostPinit *>(hv);
  for (int p = 0; p < h.np; p++) E[p] = artis_pinit::path_energy(h.T, p);
}

// The per-cell work with the vector E: checkpoints (kept), endecay_per_mass [ncell], en_cumulative [ngrid]; returns etot_simtime
double pinit_host_cells(void *hv, const double *E, double *endecay, double *en_cumulative, int nthreads) {
  HostPinit &h = *static_cast<HostPinit *>(hv);
  h.E.assign(E, E + h.np);
  h.E.push_back(0.);
  h.ckpt.assign((size_t)((artis_pinit::ncheckpoints(h.np) + 1) * h.ncell), 0.);
  h.endecay.assign((size_t)h.ncell, 0.);
  parallel_range(h.ncell, nthreads, [&](int64_t c0, int64_t c1) {
    for (int64_t c = c0; c < c1; c++) h.endecay[(size_t)c] = artis_pinit::cell_checkpoints(h.np, h.T.path_top, h.E.data(), h.X.data(), h.ncell, c, h.ckpt.data(), true);
  });
  h.en_cumulative.assign((size_t)h.G.ngrid, 0.);
  double s = 0.;
  for (int i = 0; i < h.G.ngrid; i++) {
    s += artis_pinit::cumulative_term(h.G, h.T, h.rho_tmin.data(), h.endecay.data(), i);
    h.en_cumulative[(size_t)i] = s;
  }
  if (endecay) std::memcpy(endecay, h.endecay.data(), sizeof(double) * (size_t)h.ncell);
  if (en_cumulative) std::memcpy(en_cumulative, h.en_cumulative.data(), sizeof(double) * (size_t)h.G.ngrid);
  return s;
}

// the channel of draw u in non-empty cell c after pinit_host_cells: by the checkpoints, or (full) from the whole running sum
int pinit_host_channel(const void *hv, int64_t c, float u, int full) {
  const HostPinit &h = *static_cast<const HostPinit *>(hv);
  const artis_pinit::Work W = make_work(h, 0.);
  if (!full) return artis_pinit::choose_channel(W, c, u);
  std::vector<double> cum((size_t)h.np + 2);
  return artis_pinit::choose_channel_full(W, c, u, cum.data());
}

// The population after pinit_host_cells: packets [npackets] (zeroed by the caller), channel, trials [npackets]; scal {etot_simtime,
// e_cmf_per_packet, e_cmf_total, e_ratio}. budget: the decay-time trials of one pellet_decay call (a packet is continued until it is
// complete: the result must not depend on it); returns the calls the slowest packet took, -1 when one was not complete after max_calls.
// Optional, per packet: tdecay_unit = the sum over the accepted trial's terms of meanlife * |log u| + 2 |t after the term's subtraction|
// (what a last-bit error of log moves tdecay by, in units of 2^-53, plus a last bit of every subtraction's result, whose rounding can
// fall the other way for an input that differs), margin = the smallest distance of one of its trial times from tdecaymin or tmax,
// divided by that trial's unit (how many errors of that size the acceptance is away from flipping).
int pinit_host_run(const void *hv, int64_t npackets, uint32_t seed_base, artis_packet *packets, int32_t *channel, int32_t *trials, double *scal, int budget, int max_calls,
                   double *tdecay_unit, double *margin, int nthreads) {
  const HostPinit &h = *static_cast<const HostPinit *>(hv);
  const double etot = h.en_cumulative.back();
  const artis_pinit::Work W = make_work(h, etot / (double)npackets);
  std::vector<int> calls((size_t)(nthreads > 1 ? nthreads : 1), 0);
  std::vector<int> failed(calls.size(), 0);
  const int64_t chunk = (npackets + (int64_t)calls.size() - 1) / (int64_t)calls.size();
  parallel_range(npackets, nthreads, [&](int64_t n0, int64_t n1) {
    const size_t tid = (size_t)(n0 / chunk);
    for (int64_t n = n0; n < n1; n++) {
      artis_packet &q = packets[n];
      artis_pinit::pellet_place(W, n, seed_base + (uint32_t)n, q);
      channel[n] = artis_pinit::CHANNEL_UNSET;
      trials[n] = 0;
      if (margin) {  // the same stream once more, whole: every trial time of the packet
        artis::Pkt rng;
        artis_pinit::load_rng(rng, q);
        const int ch = artis_pinit::choose_channel(W, W.G.propcell_nonemptymgi[q.cellindex], artis::rng_uniform(rng));
        margin[n] = INFINITY;
        tdecay_unit[n] = 0.;
        if (ch < h.np) {
          const double tdecaymin = !h.T.initial_packets_on ? h.T.tmin : h.T.t_model;
          const int i0 = h.T.path_start[ch], len = h.T.path_start[ch + 1] - i0 - 1;
          for (;;) {
            double t = h.T.t_model, unit = 0.;
            for (int i = 0; i < len; i++) {
              const double term = h.T.nuc_meanlife[h.T.path_nucindex[i0 + i]] * log((double)artis::rng_uniform_pos(rng));
              t -= term;
              unit += fabs(term) + 2. * fabs(t);
            }
            const double d0 = fabs(t - tdecaymin), d1 = fabs(t - h.T.tmax);
            const double m = (d0 < d1 ? d0 : d1) / unit;
            if (m < margin[n]) margin[n] = m;
            if (!(t <= tdecaymin || t >= h.T.tmax)) {
              tdecay_unit[n] = unit;
              break;
            }
          }
        }
      }
      int k = 1;
      while (!artis_pinit::pellet_decay(W, q, &channel[n], &trials[n], budget)) {
        if (k == max_calls) {
          failed[tid] = 1;
          break;
        }
        k++;
      }
      if (k > calls[tid]) calls[tid] = k;
    }
  });
  double total = 0.;
  for (int64_t n = 0; n < npackets; n++) total += packets[n].e_cmf;
  const double e_ratio = etot / total;
  for (int64_t n = 0; n < npackets; n++) artis_pinit::pellet_normalise(packets[n], e_ratio);
  scal[0] = etot, scal[1] = W.e_cmf_per_packet, scal[2] = total, scal[3] = e_ratio;
  int most = 0;
  for (size_t t = 0; t < calls.size(); t++) {
    if (failed[t]) return -1;
    if (calls[t] > most) most = calls[t];
  }
  return most;
}

}  // extern "C"
