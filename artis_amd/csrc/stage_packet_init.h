// stage_packet_init.h -- artis_amd_packet_init*: the initial pellet population made on the device and installed as the resident one
// (rules and bodies: packet_init.h).
// Kernels on the caller's stream, every output element with one writer and no float atomics: k_pinit_energy (one lane per decay path:
// its energy per mass of the top nuclide; skipped when the host hands its vector in), k_pinit_checkpoints (one lane per cell, one wave
// per workgroup as k_dep_cells: ONE walk over the paths' X lines, the running sum kept before every 64th path and at the end),
// k_pinit_cumulative (one wave: the chain over all propagation cells, every prefix stored), k_pinit_place (one lane per packet: seed,
// cell, position), k_pinit_decay (one lane per packet: channel by the cell's checkpoints, decay time, nuclide, emission, direction),
// k_pinit_gather and k_pinit_total (the packets' e_cmf side by side, then one wave: their chain in packet order, as k_dep_totals) and
// k_pinit_scale.
//
// k_pinit_decay is bounded: a lane makes at most max_trials_per_launch decay-time trials, then leaves its packet -- generator state
// in the struct, channel and trial count beside it -- on a list (one integer atomic per wave), and a further launch of the same kernel
// over that list goes on from the saved state. Every packet draws from its own generator, so the result does not depend on where it
// was cut or in which order the list was written. The host looks at the list's length between two launches; nothing waits on the device.
//
// The packets are made in a buffer of the call's own and copied over the engine's structs only when all of them are complete: a refused
// call leaves the resident population as it was.
#pragma once

namespace {

struct PinitArgs {
  artis_pinit::Work W;
  const float *rho_tmin;
  double *E, *ckpt, *endecay, *en_cumulative, *scal;  // scal: {e_cmf_total, e_ratio}
  double etot_simtime;
  artis_packet *aos;
  int64_t npackets;
  uint32_t seed_base;
  int32_t *channel, *trials;
  const int32_t *list_in;  // the parked packets a continuation launch goes on with; null: all of them
  int32_t nlist, budget;
  int32_t *list_out, *count_out, *max_trials;
  double *ecmf;  // [npackets] the packets' e_cmf, dense
};

__global__ void __launch_bounds__(BLOCK) k_pinit_energy(PinitArgs a) {
  const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (p < a.W.T.npaths) a.E[p] = artis_pinit::path_energy(a.W.T, (int)p);
}

// one wave per workgroup. A lane past the last cell walks the last cell's lines (in bounds, no divergence in the loop) and stores nothing.
__global__ void __launch_bounds__(64) k_pinit_checkpoints(PinitArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool mine = c < a.W.ncell;
  const int64_t cc = mine ? c : a.W.ncell - 1;
  const double total = artis_pinit::cell_checkpoints(a.W.T.npaths, a.W.T.path_top, a.E, a.W.X, a.W.ncell, cc, a.ckpt, mine);
  if (mine) a.endecay[c] = total;
}

// en_cumulative[i] = the sequential sum of the terms 0 .. i from +0.0, by one wave: the lanes form 64 terms at a time (the next 64 while
// the current ones are added), every lane adds them in order and keeps the sum as it stood after its own term. (A term past the end is
// +0.0, which changes no non-negative sum.)
__global__ void __launch_bounds__(64) k_pinit_cumulative(PinitArgs a) {
  const int lane = threadIdx.x;
  const int64_t n = a.W.G.ngrid;
  const auto term = [&](int64_t i) { return artis_pinit::cumulative_term(a.W.G, a.W.T, a.rho_tmin, a.endecay, (int)i); };
  double s = 0.;
  double t = lane < n ? term(lane) : 0.;
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t inext = base + 64 + lane;
    const double tn = inext < n ? term(inext) : 0.;
    double prefix = 0.;
#pragma unroll
    for (int j = 0; j < 64; j++) {
      s += readlane_f64(t, j);
      if (j == lane) prefix = s;
    }
    if (base + lane < n) a.en_cumulative[base + lane] = prefix;
    t = tn;
  }
}

__global__ void __launch_bounds__(BLOCK) k_pinit_place(PinitArgs a) {
  const int64_t n = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (n >= a.npackets) return;
  artis_pinit::pellet_place(a.W, n, a.seed_base + (uint32_t)n, a.aos[n]);
  a.channel[n] = artis_pinit::CHANNEL_UNSET;
  a.trials[n] = 0;
}

__global__ void __launch_bounds__(BLOCK) k_pinit_decay(PinitArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int64_t n = -1;
  if (a.list_in) {
    if (i < a.nlist) n = a.list_in[i];
  } else if (i < a.npackets) {
    n = i;
  }
  bool parked = false;
  int32_t trials = 0;
  if (n >= 0) {
    trials = a.trials[n];
    int32_t channel = a.channel[n];
    parked = !artis_pinit::pellet_decay(a.W, a.aos[n], &channel, &trials, a.budget);
    a.channel[n] = channel;
    a.trials[n] = trials;
  }
  // the wave's largest trial count and its parked packets: one integer atomic each per wave
  int32_t m = trials;
  for (int off = 32; off > 0; off >>= 1) {
    const int32_t o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  const int lane = threadIdx.x & 63;
  if (lane == 0 && m > 0) atomicMax(a.max_trials, m);
  const unsigned long long mask = __ballot(parked);
  if (mask == 0) return;
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(a.count_out, __popcll(mask));
  base = __shfl(base, leader);
  if (parked) a.list_out[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)n;
}

// the packets' e_cmf side by side: what the chain below reads (a struct is 256 bytes: read in place, a wave's load would touch 64 lines)
__global__ void __launch_bounds__(BLOCK) k_pinit_gather(PinitArgs a) {
  const int64_t n = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (n < a.npackets) a.ecmf[n] = a.aos[n].e_cmf;
}

// packet.cc:149-151: the sequential sum of e_cmf in packet order from +0.0 by one wave, as dep_wave_chain, with the loads of the next
// TOTAL_AHEAD x 64 terms in flight while the current ones are added (1e7 terms: the chain runs at the latency of its additions, not of
// its loads). A term past the end is +0.0, which changes no non-negative sum.
constexpr int TOTAL_AHEAD = 4;
__global__ void __launch_bounds__(64) k_pinit_total(PinitArgs a) {
  const int lane = threadIdx.x;
  const int64_t n = a.npackets;
  const auto load = [&](int64_t base, double t[TOTAL_AHEAD]) {
#pragma unroll
    for (int k = 0; k < TOTAL_AHEAD; k++) {
      const int64_t i = base + 64 * k + lane;
      t[k] = i < n ? a.ecmf[i] : 0.;
    }
  };
  double s = 0.;
  double t[TOTAL_AHEAD], tn[TOTAL_AHEAD];
  load(0, t);
  for (int64_t base = 0; base < n; base += 64 * TOTAL_AHEAD) {
    load(base + 64 * TOTAL_AHEAD, tn);
#pragma unroll
    for (int k = 0; k < TOTAL_AHEAD; k++) {
#pragma unroll
      for (int j = 0; j < 64; j++) s += readlane_f64(t[k], j);
    }
#pragma unroll
    for (int k = 0; k < TOTAL_AHEAD; k++) t[k] = tn[k];
  }
  if (lane == 0) {
    a.scal[0] = s;
    a.scal[1] = a.etot_simtime / s;
  }
}

__global__ void __launch_bounds__(BLOCK) k_pinit_scale(PinitArgs a) {
  const int64_t n = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (n < a.npackets) artis_pinit::pellet_normalise(a.aos[n], a.scal[1]);
}

// everything of artis_amd_packet_init*: the tables and the per-cell arrays in one block made by the set-up; what a call leaves for the
// download (every packet's channel and trial count) in a block of its own, replaced by the next call
struct PinitState {
  StageBlock block;
  StageBlock *kept = nullptr;
  hipEvent_t ev[ARTIS_PINIT_NKERNELS + 1] = {};
  int64_t ncell = 0, npackets = 0;
  int32_t ngrid = 0, npaths = 0, nck = 0, max_trials_per_launch = artis_pinit::DEFAULT_TRIALS_PER_LAUNCH;
  artis_pinit::Tables T{};  // device pointers
  artis_pinit::Grid G{};
  int32_t *d_path_top = nullptr, *d_gamma_start = nullptr, *d_counts = nullptr;  // counts: the two lists' lengths, the largest trial count
  double *d_endecay_gamma = nullptr, *d_endecay_particle = nullptr, *d_probsum = nullptr, *d_gamma_energy = nullptr, *d_gamma_prob = nullptr, *d_initq = nullptr;
  double *d_E = nullptr, *d_ckpt = nullptr, *d_endecay = nullptr, *d_encum = nullptr, *d_scal = nullptr;
  int32_t *d_channel = nullptr, *d_trials = nullptr;  // in *kept
  double etot_simtime = 0., e_cmf_per_packet = 0., e_cmf_total = 0., e_ratio = 0.;
  int32_t continuation_launches = 0, max_trials = 0;
  double kernel_ms[ARTIS_PINIT_NKERNELS] = {};
  bool valid = false;
  ~PinitState() {
    delete kept;
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

void pinit_free(PinitState *st) { delete st; }

}  // namespace

extern "C" {

int artis_amd_packet_init_setup(artis_amd_engine *e, const artis_packet_init_model *m) {
  if (!e || !m) return stage_error(ARTIS_ERR_ARG, "packet_init: null engine or model");
  STAGE_STRUCT_SIZE(m, artis_packet_init_model, "packet_init");
  if (!e->decay) return stage_error(ARTIS_ERR_ARG, "packet_init: no network (artis_amd_decay_setup)");
  if (!e->dep) return stage_error(ARTIS_ERR_ARG, "packet_init: no energies (artis_amd_deposition_setup)");
  const DecayState *dc = e->decay;
  const DepState *dp = e->dep;
  const int64_t n = dc->ncell;
  const int nn = dc->T.nnuclides, np = dc->T.npaths;
  bool unsupported = false;
  const std::string bad = artis_pinit::packet_init_validate(*m, nn, n, dc->h_meanlife.data(), e->model_copy.tmin, dc->t_model, &unsupported);
  if (!bad.empty()) return stage_error(unsupported ? ARTIS_ERR_UNSUPPORTED : ARTIS_ERR_ARG, "packet_init: " + bad);
  HIP_TRY(hipSetDevice(e->device));
  pinit_free(e->pinit);  // a second set-up replaces the first
  e->pinit = nullptr;
  PinitState *st = new PinitState();
  st->ncell = n;
  st->ngrid = e->Mh.ngrid;
  st->npaths = np;
  st->nck = artis_pinit::ncheckpoints(np);
  if (m->max_trials_per_launch > 0) st->max_trials_per_launch = m->max_trials_per_launch;
  const int64_t nlines = nn > 0 ? m->gamma_start[nn] : 0;
  const bool channel = m->initial_packets_on && m->use_model_initial_energy;
  const int rc = st->block.make(
      {piece(&st->d_path_top, np), piece(&st->d_gamma_start, (int64_t)nn + 1), piece(&st->d_counts, 4), piece(&st->d_endecay_gamma, nn),
       piece(&st->d_endecay_particle, (int64_t)nn * artis_pinit::NDECAYTYPES), piece(&st->d_probsum, nn), piece(&st->d_gamma_energy, nlines),
       piece(&st->d_gamma_prob, nlines), piece(&st->d_initq, channel ? n : 0), piece(&st->d_E, np), piece(&st->d_ckpt, ((int64_t)st->nck + 1) * n),
       piece(&st->d_endecay, n), piece(&st->d_encum, st->ngrid), piece(&st->d_scal, 2)},
      "packet_init", "the tables and the cells' checkpoints");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  e->pinit = st;
  for (hipEvent_t &ev : st->ev) HIP_TRY(hipEventCreate(&ev));
  const hipMemcpyKind up = hipMemcpyHostToDevice;
  HIP_TRY(stage_copy(st->d_path_top, dc->h_path_top.data(), np, up));
  HIP_TRY(stage_copy(st->d_gamma_start, m->gamma_start, (int64_t)nn + 1, up));
  HIP_TRY(stage_copy(st->d_endecay_gamma, dp->h_endecay_gamma.data(), nn, up));
  HIP_TRY(stage_copy(st->d_endecay_particle, dp->h_endecay_particle.data(), (int64_t)nn * artis_pinit::NDECAYTYPES, up));
  HIP_TRY(stage_copy(st->d_probsum, m->nuc_decay_daughters_probsum, nn, up));
  HIP_TRY(stage_copy(st->d_gamma_energy, m->gamma_energy, nlines, up));
  HIP_TRY(stage_copy(st->d_gamma_prob, m->gamma_probability, nlines, up));
  if (channel) HIP_TRY(stage_copy(st->d_initq, m->initenergyq, n, up));
  artis_pinit::Tables &T = st->T;
  T.nnuclides = nn;
  T.npaths = np;
  T.path_start = dc->d_path_start;
  T.path_nucindex = dc->d_path_nuc;
  T.path_last_decaytype = dc->d_path_type;
  T.path_top = st->d_path_top;
  T.path_lambda = dc->d_path_lambda;
  T.path_branchproduct = dc->d_path_branch;
  T.nuc_meanlife = dp->d_meanlife;
  T.nuc_mass = dc->d_nuc_mass;
  T.endecay_gamma = st->d_endecay_gamma;
  T.endecay_particle = st->d_endecay_particle;
  T.probsum = st->d_probsum;
  T.gamma_start = st->d_gamma_start;
  T.gamma_energy = st->d_gamma_energy;
  T.gamma_probability = st->d_gamma_prob;
  T.initenergyq = channel ? st->d_initq : nullptr;
  T.t_model = dc->t_model;
  T.tmin = e->model_copy.tmin;
  T.tmax = m->tmax;
  T.initial_packets_on = m->initial_packets_on ? 1 : 0;
  artis_pinit::Grid &G = st->G;
  G.gridtype = e->Mh.gridtype;
  G.ngrid = e->Mh.ngrid;
  for (int a = 0; a < 3; a++) {
    G.ncoordgrid[a] = e->Mh.ncoordgrid[a];
    G.coordstride[a] = e->Mh.coordstride[a];
    G.coord_pos_min_tmin[a] = e->M.coord_pos_min_tmin[a];
  }
  G.propcell_nonemptymgi = e->M.propcell_nonemptymgi;
  G.rmax = e->model_copy.rmax;
  G.tmin = e->model_copy.tmin;
  return ARTIS_OK;
}

int artis_amd_packet_init(artis_amd_engine *e, int64_t npackets, uint32_t seed_base, const double *energy_vector, void *hip_stream) {
  if (!e) return stage_error(ARTIS_ERR_ARG, "packet_init: null engine");
  if (!e->pinit || !e->decay || !e->dep) return stage_error(ARTIS_ERR_ARG, "packet_init: no set-up (artis_amd_packet_init_setup)");
  if (npackets < 1 || npackets > 2147483000LL) return stage_error(ARTIS_ERR_ARG, "packet_init: npackets must be between 1 and 2147483000");
  PinitState *st = e->pinit;
  const int64_t n = st->ncell;
  const int np = st->npaths;
  if (n < 1 || st->ngrid < 1) return stage_error(ARTIS_ERR_ARG, "packet_init: etot_simtime is not positive (a grid without a non-empty cell)");
  if (energy_vector) {
    const std::string bad = artis_pinit::energy_vector_validate(energy_vector, np);
    if (!bad.empty()) return stage_error(ARTIS_ERR_ARG, "packet_init: energy_vector: " + bad);
  }
  HIP_TRY(hipSetDevice(e->device));
  st->valid = false;
  hipStream_t s = (hipStream_t)hip_stream;
  // what the call leaves behind (channel, trials) and what it only works with (the packets before they are installed, the two lists)
  StageBlock *kept = new StageBlock();
  int32_t *d_channel = nullptr, *d_trials = nullptr, *d_list[2] = {};
  artis_packet *d_new = nullptr;
  double *d_ecmf = nullptr;
  StageBlock work;
  int rc = kept->make({piece(&d_channel, npackets), piece(&d_trials, npackets)}, "packet_init", "the packets' channels");
  if (rc == ARTIS_OK) rc = work.make({piece(&d_new, npackets), piece(&d_list[0], npackets), piece(&d_list[1], npackets), piece(&d_ecmf, npackets)}, "packet_init", "the new packets");
  if (rc != ARTIS_OK) {
    delete kept;
    return rc;
  }
  delete st->kept;
  st->kept = kept;
  st->d_channel = d_channel;
  st->d_trials = d_trials;
  st->npackets = npackets;

  PinitArgs a{};
  a.W.T = st->T;
  a.W.G = st->G;
  a.W.E = st->d_E;
  a.W.X = e->decay->d_X;
  a.W.ncell = n;
  a.W.ckpt = st->d_ckpt;
  a.W.en_cumulative = st->d_encum;
  a.rho_tmin = e->decay->d_rho_tmin;
  a.E = st->d_E;
  a.ckpt = st->d_ckpt;
  a.endecay = st->d_endecay;
  a.en_cumulative = st->d_encum;
  a.scal = st->d_scal;
  a.aos = d_new;
  a.ecmf = d_ecmf;
  a.npackets = npackets;
  a.seed_base = seed_base;
  a.channel = d_channel;
  a.trials = d_trials;
  a.budget = st->max_trials_per_launch;
  a.max_trials = st->d_counts + 2;
  auto done = [&](const char *kernel) -> int {
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("packet_init: ") + kernel + ": " + hipGetErrorString(err));
    return ARTIS_OK;
  };
  HIP_TRY(hipMemsetAsync(st->d_counts, 0, sizeof(int32_t) * 4, s));
  HIP_TRY(hipEventRecord(st->ev[0], s));
  if (energy_vector) {
    HIP_TRY(stage_copy(st->d_E, energy_vector, np, hipMemcpyHostToDevice, &s));
    HIP_TRY(hipStreamSynchronize(s));  // (the caller's array is free again)
  } else if (np > 0) {
    hipLaunchKernelGGL(k_pinit_energy, dim3(nblocks(np)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_pinit_energy")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->ev[1], s));
  hipLaunchKernelGGL(k_pinit_checkpoints, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a);
  if ((rc = done("k_pinit_checkpoints")) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->ev[2], s));
  hipLaunchKernelGGL(k_pinit_cumulative, dim3(1), dim3(64), 0, s, a);
  if ((rc = done("k_pinit_cumulative")) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->ev[3], s));
  double etot = 0.;
  HIP_TRY(stage_copy(&etot, st->d_encum + (st->ngrid - 1), 1, hipMemcpyDeviceToHost));
  if (!(etot > 0.) || !std::isfinite(etot)) return stage_error(ARTIS_ERR_ARG, "packet_init: etot_simtime is not positive and finite");
  st->etot_simtime = etot;
  st->e_cmf_per_packet = etot / (double)npackets;
  a.etot_simtime = etot;
  a.W.e_cmf_per_packet = st->e_cmf_per_packet;
  hipLaunchKernelGGL(k_pinit_place, dim3(nblocks(npackets)), dim3(BLOCK), 0, s, a);
  if ((rc = done("k_pinit_place")) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->ev[4], s));
  // the first launch over all packets, then the parked ones until none is left
  int32_t nparked = 0;
  int launches = 0;
  for (int k = 0;; k ^= 1) {
    a.list_out = d_list[k];
    a.count_out = st->d_counts + k;
    HIP_TRY(hipMemsetAsync(a.count_out, 0, sizeof(int32_t), s));
    const int64_t nwork = a.list_in ? nparked : npackets;
    hipLaunchKernelGGL(k_pinit_decay, dim3(nblocks(nwork)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_pinit_decay")) != ARTIS_OK) return rc;
    HIP_TRY(stage_copy(&nparked, a.count_out, 1, hipMemcpyDeviceToHost));
    if (nparked == 0) break;
    if (launches == artis_pinit::MAX_CONTINUATION_LAUNCHES) {
      int32_t first = 0, path = -1;
      HIP_TRY(stage_copy(&first, d_list[k], 1, hipMemcpyDeviceToHost));
      HIP_TRY(stage_copy(&path, d_channel + first, 1, hipMemcpyDeviceToHost));
      st->continuation_launches = launches;
      return stage_error(ARTIS_ERR_NOTCONVERGED, "packet_init: path " + std::to_string(path) + ": no decay time of packet " + std::to_string(first) + " between tmin and tmax after " +
                                                     std::to_string(launches) + " continuation launches of " + std::to_string(a.budget) + " trials (" + std::to_string(nparked) +
                                                     " packets left); the resident population is unchanged");
    }
    launches++;
    a.list_in = d_list[k];
    a.nlist = nparked;
  }
  st->continuation_launches = launches;
  HIP_TRY(hipEventRecord(st->ev[5], s));
  hipLaunchKernelGGL(k_pinit_gather, dim3(nblocks(npackets)), dim3(BLOCK), 0, s, a);
  if ((rc = done("k_pinit_gather")) != ARTIS_OK) return rc;
  hipLaunchKernelGGL(k_pinit_total, dim3(1), dim3(64), 0, s, a);
  if ((rc = done("k_pinit_total")) != ARTIS_OK) return rc;
  hipLaunchKernelGGL(k_pinit_scale, dim3(nblocks(npackets)), dim3(BLOCK), 0, s, a);
  if ((rc = done("k_pinit_scale")) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->ev[6], s));
  double scal[2] = {};
  HIP_TRY(stage_copy(scal, st->d_scal, 2, hipMemcpyDeviceToHost));
  if (!std::isfinite(scal[0]) || !(scal[0] > 0.)) return stage_error(ARTIS_ERR_ARG, "packet_init: the packets' energy sum is not positive and finite");
  st->e_cmf_total = scal[0];
  st->e_ratio = scal[1];
  HIP_TRY(stage_copy(&st->max_trials, st->d_counts + 2, 1, hipMemcpyDeviceToHost));
  // the population is complete: it replaces the resident one
  if ((rc = ensure_packet_buffers(e, npackets)) != ARTIS_OK) return rc;
  if ((rc = ensure_aos(e, npackets)) != ARTIS_OK) return rc;
  HIP_TRY(hipMemcpyAsync(e->d_aos, d_new, sizeof(artis_packet) * (size_t)npackets, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = install_resident_aos(e, npackets)) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->ev[7], s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < ARTIS_PINIT_NKERNELS; k++) {
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, st->ev[k], st->ev[k + 1]));
    st->kernel_ms[k] = f;
  }
  st->valid = true;
  return ARTIS_OK;
}

int artis_amd_packet_init_download(artis_amd_engine *e, artis_packet_init_result *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "packet_init: null argument");
  STAGE_STRUCT_SIZE(out, artis_packet_init_result, "packet_init");
  if (!e->pinit || !e->pinit->valid) return stage_error(ARTIS_ERR_ARG, "packet_init: nothing made (artis_amd_packet_init)");
  PinitState *st = e->pinit;
  HIP_TRY(hipSetDevice(e->device));
  const hipMemcpyKind down = hipMemcpyDeviceToHost;
  HIP_TRY(stage_copy(out->en_cumulative, st->d_encum, st->ngrid, down));
  HIP_TRY(stage_copy(out->energy_vector, st->d_E, st->npaths, down));
  HIP_TRY(stage_copy(out->endecay_per_mass, st->d_endecay, st->ncell, down));
  HIP_TRY(stage_copy(out->channel, st->d_channel, st->npackets, down));
  HIP_TRY(stage_copy(out->trials, st->d_trials, st->npackets, down));
  out->npackets = st->npackets;
  out->ngrid = st->ngrid;
  out->npts_nonempty = (int32_t)st->ncell;
  out->npaths = st->npaths;
  out->ncheckpoints = st->nck;
  out->etot_simtime = st->etot_simtime;
  out->e_cmf_per_packet = st->e_cmf_per_packet;
  out->e_cmf_total = st->e_cmf_total;
  out->e_ratio = st->e_ratio;
  out->continuation_launches = st->continuation_launches;
  out->max_trials = st->max_trials;
  for (int k = 0; k < ARTIS_PINIT_NKERNELS; k++) out->kernel_ms[k] = st->kernel_ms[k];
  return ARTIS_OK;
}

}  // extern "C"
