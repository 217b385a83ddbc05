// stage_deposition.h -- artis_amd_deposition_*: the deposition rates, the grey depth and the thickness flags of the grid update (rules
// and bodies: deposition.h), and artis_amd_grid_update_deposited, which hands the flags with the decay update's matter to the ion
// balance (stage_ionbal.h) without the host.
// Kernels on the caller's stream, every output element with one writer: k_dep_powers (one lane per (nuclide, vector): its own share,
// then the paths whose top it is, in path order; skipped when the host hands its vectors in), k_dep_pack (the five channels of the
// radioactive nuclides side by side, in the order of the walk), k_dep_cells (one lane per cell: ONE pass over the radioactive
// nuclides' X lines feeds the five channel sums; then the cell's estimators, outputs, grey depth and flag), k_dep_totals (one wave
// per chain: the four cell sums and the eleven products with totmassnuclide), k_dep_totmass (set-up, one wave per nuclide).
//
// k_dep_cells runs in one-wave workgroups: the bench grid's 65 752 cells are 1 028 waves for 256 CUs with 4 SIMDs each, and single
// waves are dealt over every CU and SIMD (four per CU, one per SIMD) where 256-thread workgroups would leave the 257th as a second
// workgroup on one CU. X is [nuclide][cell]: the 64 lanes read one 256-byte line per nuclide; the nuclide's index and its five powers
// are indexed by the loop counter only and load through the scalar unit. The lane has DEP_DEPTH lines in flight before the first
// addition; the additions stay sequential per channel, in nuclide order.
#pragma once

namespace {

struct DepArgs {
  artis_dep::Tables T;
  artis_dep::Step S;
  artis_dep::Estimators E;
  artis_dep::CellOut out;
  int64_t ncell;
  const float *X, *rho, *rho_tmin, *kappagrey;
  const double *coef, *surv, *assocvol, *radial;
  double *vectors, *pw, *totmass, *totals;  // vectors [NVECTORS][nnuclides]; pw [nrad][NCHANNELS]; totmass [nnuclides + 1] (the last: mtot)
};

__global__ void __launch_bounds__(BLOCK) k_dep_powers(DepArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (int64_t)artis_dep::NVECTORS * a.T.nnuclides) return;
  const int v = (int)(i / a.T.nnuclides);
  a.vectors[i] = artis_dep::power_entry(a.T, a.coef, a.surv, v, (int)(i - (int64_t)v * a.T.nnuclides));
}

__global__ void __launch_bounds__(BLOCK) k_dep_pack(DepArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (int64_t)artis_dep::NCHANNELS * a.T.nrad) return;
  const int k = (int)(i / artis_dep::NCHANNELS), ch = (int)(i - (int64_t)k * artis_dep::NCHANNELS);
  a.pw[i] = a.vectors[(int64_t)ch * a.T.nnuclides + a.T.rad_nuc[k]];
}

// one wave per workgroup. A lane past the last cell walks the last cell's lines (in bounds, no divergence in the loop) and stores nothing.
__global__ void __launch_bounds__(64) k_dep_cells(DepArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t cc = c < a.ncell ? c : a.ncell - 1;
  double sum[artis_dep::NCHANNELS];
  artis_dep::cell_power_sums(a.T, a.pw, a.X, a.ncell, cc, sum);
  if (c < a.ncell) artis_dep::cell_entry(sum, a.S, a.E, a.rho, a.kappagrey, a.assocvol, a.radial, a.ncell, c, a.out);  // (stores last: the table loads above stay scalar)
}

// the sequential sum of term(0), term(1), ... term(n - 1) from +0.0 by one wave: the lanes form 64 terms at a time (the next 64 while
// the current ones are added) and every lane adds them in order, so each lane holds the same sum
template <class F>
__device__ inline double dep_wave_chain(const int64_t n, const int lane, F term) {
  double s = 0.;
  double t = lane < n ? term((int64_t)lane) : 0.;
  for (int64_t base = 0; base < n; base += 64) {
    const int64_t inext = base + 64 + lane;
    const double tn = inext < n ? term(inext) : 0.;
    const int64_t left = n - base;
    if (left >= 64) {
#pragma unroll
      for (int j = 0; j < 64; j++) s += readlane_f64(t, j);
    } else {
#pragma unroll
      for (int j = 0; j < 64; j++)
        if (j < left) s += readlane_f64(t, j);
    }
    t = tn;
  }
  return s;
}

__global__ void __launch_bounds__(64) k_dep_totals(DepArgs a) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const double s = dep_wave_chain(artis_dep::total_length(a.T, a.ncell, k), lane,
                                  [&](int64_t i) { return artis_dep::total_term(a.T, a.E, a.S.nprocs, a.vectors, a.totmass, k, i); });
  if (lane == 0) a.totals[k] = s;
}

// chain b: totmassnuclide[b] for b < nnuclides, mtot for b == nnuclides (set-up, once)
__global__ void __launch_bounds__(64) k_dep_totmass(DepArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nuc = b < a.T.nnuclides ? b : -1;
  const double s = dep_wave_chain(a.ncell, lane, [&](int64_t c) { return artis_dep::totmass_term(a.rho_tmin, a.assocvol, a.X, a.ncell, c, nuc); });
  if (lane == 0) a.totmass[b] = s;
}

// everything of artis_amd_deposition_*: one block made by the set-up
struct DepState {
  StageBlock block;
  int64_t ncell = 0;
  artis_dep::Tables T{};  // device pointers
  double *d_meanlife = nullptr, *d_energy = nullptr, *d_assocvol = nullptr, *d_radial = nullptr;
  int32_t *d_top_start = nullptr, *d_top_path = nullptr, *d_top_end = nullptr, *d_rad_nuc = nullptr;
  double *d_vectors = nullptr, *d_pw = nullptr, *d_totmass = nullptr, *d_totals = nullptr;
  double *d_cell = nullptr;  // eps_ana [5][n] | dep [5][n] | ntlepton [n]
  float *d_grey = nullptr;
  int32_t *d_thick = nullptr;
  double t_mid = 0.;
  int32_t nts_next = 0;
  uint64_t decay_serial = 0;  // the decay update this one was made on
  bool valid = false;
  double kernel_ms[3] = {};
  std::vector<double> h_endecay_gamma, h_endecay_particle;  // [nnuclides], [nnuclides][6] as handed in: what artis_amd_packet_init_setup reads
};

void dep_free(DepState *st) { delete st; }

DepArgs dep_args(const artis_amd_engine *e) {
  const DepState *st = e->dep;
  const DecayState *dc = e->decay;
  DepArgs a{};
  a.T = st->T;
  a.ncell = st->ncell;
  a.X = dc->d_X;
  a.rho = dc->d_rho;
  a.rho_tmin = dc->d_rho_tmin;
  a.kappagrey = e->C.kappagrey;
  a.coef = dc->d_coef;
  a.surv = dc->d_surv;
  a.assocvol = st->d_assocvol;
  a.radial = st->d_radial;
  a.vectors = st->d_vectors;
  a.pw = st->d_pw;
  a.totmass = st->d_totmass;
  a.totals = st->d_totals;
  a.E.raw[0] = e->E.dep_estimator_gamma;
  a.E.raw[1] = e->E.dep_estimator_positron;
  a.E.raw[2] = e->E.dep_estimator_electron;
  a.E.raw[3] = e->E.dep_estimator_alpha;
  a.E.est_stride = 8;
  a.out.eps_ana = st->d_cell;
  a.out.dep = st->d_cell ? st->d_cell + artis_dep::NCHANNELS * st->ncell : nullptr;
  a.out.ntlepton = st->d_cell ? st->d_cell + 2 * artis_dep::NCHANNELS * st->ncell : nullptr;
  a.out.grey_depth = st->d_grey;
  a.out.thick = st->d_thick;
  return a;
}

}  // namespace

extern "C" {

int artis_amd_deposition_setup(artis_amd_engine *e, const artis_deposition_model *m) {
  if (!e || !m) return stage_error(ARTIS_ERR_ARG, "deposition: null engine or model");
  STAGE_STRUCT_SIZE(m, artis_deposition_model, "deposition");
  if (!e->decay) return stage_error(ARTIS_ERR_ARG, "deposition: no network (artis_amd_decay_setup)");
  const DecayState *dc = e->decay;
  const int64_t n = dc->ncell;
  const int nn = dc->T.nnuclides, np = dc->T.npaths;
  std::string bad = artis_dep::deposition_validate(*m, nn, n);
  if (!bad.empty()) return stage_error(ARTIS_ERR_ARG, "deposition: " + bad);
  const artis_dep::Rows r = artis_dep::build_dep_rows(*m, nn, np, dc->h_path_top.data(), dc->h_path_end.data(), dc->h_meanlife.data(), &bad);
  if (!bad.empty()) return stage_error(ARTIS_ERR_ARG, "deposition: " + bad);
  HIP_TRY(hipSetDevice(e->device));
  dep_free(e->dep);  // a second set-up replaces the first
  e->dep = nullptr;
  pinit_free(e->pinit);  // ... and the pellet set-up that was made on the first goes with it
  e->pinit = nullptr;
  DepState *st = new DepState();
  st->ncell = n;
  const int64_t nrad = (int64_t)r.rad_nuc.size(), nv = artis_dep::NVECTORS, nch = artis_dep::NCHANNELS;
  const int rc = st->block.make(
      {piece(&st->d_meanlife, nn), piece(&st->d_energy, nv * nn), piece(&st->d_assocvol, n), piece(&st->d_radial, n), piece(&st->d_top_start, (int64_t)nn + 1),
       piece(&st->d_top_path, np), piece(&st->d_top_end, np), piece(&st->d_rad_nuc, nrad), piece(&st->d_vectors, nv * nn), piece(&st->d_pw, nch * nrad),
       piece(&st->d_totmass, (int64_t)nn + 1), piece(&st->d_totals, artis_dep::NTOTALS), piece(&st->d_cell, (2 * nch + 1) * n), piece(&st->d_grey, n),
       piece(&st->d_thick, n)},
      "deposition", "the tables and the result block");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  e->dep = st;
  st->h_endecay_gamma.assign(m->nuc_endecay_gamma, m->nuc_endecay_gamma + nn);
  st->h_endecay_particle.assign(m->nuc_endecay_particle, m->nuc_endecay_particle + (int64_t)nn * artis_dep::NQDOT);
  const hipMemcpyKind up = hipMemcpyHostToDevice;
  HIP_TRY(stage_copy(st->d_meanlife, dc->h_meanlife.data(), nn, up));
  HIP_TRY(stage_copy(st->d_energy, r.energy.data(), nv * nn, up));
  HIP_TRY(stage_copy(st->d_assocvol, m->assocvolume_tmin, n, up));
  HIP_TRY(stage_copy(st->d_radial, m->radial_pos_tmin, n, up));
  HIP_TRY(stage_copy(st->d_top_start, r.top_start.data(), (int64_t)nn + 1, up));
  HIP_TRY(stage_copy(st->d_top_path, r.top_path.data(), np, up));
  HIP_TRY(stage_copy(st->d_top_end, r.top_end.data(), np, up));
  HIP_TRY(stage_copy(st->d_rad_nuc, r.rad_nuc.data(), nrad, up));
  artis_dep::Tables &T = st->T;
  T.nnuclides = nn;
  T.npaths = np;
  T.nrad = (int32_t)nrad;
  T.nuc_meanlife = st->d_meanlife;
  T.nuc_mass = dc->d_nuc_mass;
  T.energy = st->d_energy;
  T.top_start = st->d_top_start;
  T.top_path = st->d_top_path;
  T.top_end = st->d_top_end;
  T.rad_nuc = st->d_rad_nuc;
  if (n > 0) {
    hipLaunchKernelGGL(k_dep_totmass, dim3((unsigned)(nn + 1)), dim3(64), 0, nullptr, dep_args(e));
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("deposition: k_dep_totmass: ") + hipGetErrorString(err));
  }
  return ARTIS_OK;
}

int artis_amd_deposition_update(artis_amd_engine *e, const artis_deposition_params *p, void *hip_stream) {
  if (!e || !p) return stage_error(ARTIS_ERR_ARG, "deposition: null engine or parameters");
  STAGE_STRUCT_SIZE(p, artis_deposition_params, "deposition");
  if (!e->decay) return stage_error(ARTIS_ERR_ARG, "deposition: no network (artis_amd_decay_setup)");
  if (!e->dep) return stage_error(ARTIS_ERR_ARG, "deposition: no energies (artis_amd_deposition_setup)");
  if (!e->decay->valid) return stage_error(ARTIS_ERR_ARG, "deposition: no decay update (artis_amd_decay_update)");
  if (!e->have_cells) return stage_error(ARTIS_ERR_ARG, "deposition: no cell state (artis_amd_set_cellstate)");
  if (!(p->mid > 0.) || !(p->width > 0.) || !std::isfinite(p->mid) || !std::isfinite(p->width) || p->nprocs < 1)
    return stage_error(ARTIS_ERR_ARG, "deposition: mid and width must be positive and finite, nprocs at least 1");
  if (std::isnan(p->optical_depth_is_thick) || (ARTIS_OPT_VPKT_ON && std::isnan(p->optical_depth_is_thick_vpkt)))
    return stage_error(ARTIS_ERR_ARG, "deposition: optical_depth_is_thick is not a number");
  DepState *st = e->dep;
  const DecayState *dc = e->decay;
  const int64_t n = st->ncell, nn = st->T.nnuclides, nrad = st->T.nrad;
  if (p->power_vectors) {
    const std::string bad = artis_dep::vectors_validate(p->power_vectors, (int)nn, dc->h_meanlife.data());
    if (!bad.empty()) return stage_error(ARTIS_ERR_ARG, "deposition: power_vectors: " + bad);
  }
  HIP_TRY(hipSetDevice(e->device));
  st->valid = false;
  hipStream_t s = (hipStream_t)hip_stream;
  DepArgs a = dep_args(e);
  a.S.t_mid = dc->t_mid;
  a.S.tmin = e->model_copy.tmin;
  a.S.rmax = e->model_copy.rmax;
  a.S.prev_mid = p->mid;
  a.S.prev_width = p->width;
  a.S.nprocs = p->nprocs;
  a.S.nts_next = p->nts_next;
  a.S.num_grey_timesteps = p->num_grey_timesteps;
  a.S.optical_depth_is_thick = p->optical_depth_is_thick;
  a.S.optical_depth_is_thick_vpkt = p->optical_depth_is_thick_vpkt;
  auto done = [&](const char *kernel) -> int {
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("deposition: ") + kernel + ": " + hipGetErrorString(err));
    return ARTIS_OK;
  };
  int rc;
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  if (p->power_vectors) {
    HIP_TRY(stage_copy(st->d_vectors, p->power_vectors, artis_dep::NVECTORS * nn, hipMemcpyHostToDevice, &s));
    HIP_TRY(hipStreamSynchronize(s));  // (the caller's array is free again)
  } else if (nn > 0) {
    hipLaunchKernelGGL(k_dep_powers, dim3(nblocks(artis_dep::NVECTORS * nn)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_dep_powers")) != ARTIS_OK) return rc;
  }
  if (nrad > 0) {
    hipLaunchKernelGGL(k_dep_pack, dim3(nblocks(artis_dep::NCHANNELS * nrad)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_dep_pack")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[1], s));
  if (n > 0) {
    hipLaunchKernelGGL(k_dep_cells, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a);
    if ((rc = done("k_dep_cells")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[2], s));
  hipLaunchKernelGGL(k_dep_totals, dim3(artis_dep::NTOTALS), dim3(64), 0, s, a);
  if ((rc = done("k_dep_totals")) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->block.ev[3], s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) HIP_TRY(st->block.elapsed_ms(k, &st->kernel_ms[k]));
  st->t_mid = dc->t_mid;
  st->nts_next = p->nts_next;
  st->decay_serial = dc->serial;
  st->valid = true;
  return ARTIS_OK;
}

int artis_amd_deposition_download(artis_amd_engine *e, artis_deposition_result *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "deposition: null argument");
  STAGE_STRUCT_SIZE(out, artis_deposition_result, "deposition");
  if (!e->dep || !e->dep->valid) return stage_error(ARTIS_ERR_ARG, "deposition: nothing updated (artis_amd_deposition_update)");
  DepState *st = e->dep;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell, nn = st->T.nnuclides, nch = artis_dep::NCHANNELS;
  const hipMemcpyKind down = hipMemcpyDeviceToHost;
  HIP_TRY(stage_copy(out->eps_ana, st->d_cell, nch * n, down));
  HIP_TRY(stage_copy(out->dep, st->d_cell ? st->d_cell + nch * n : nullptr, nch * n, down));
  HIP_TRY(stage_copy(out->ntlepton_deposition_rate_density, st->d_cell ? st->d_cell + 2 * nch * n : nullptr, n, down));
  HIP_TRY(stage_copy(out->grey_depth, st->d_grey, n, down));
  HIP_TRY(stage_copy(out->thick, st->d_thick, n, down));
  HIP_TRY(stage_copy(out->power_vectors, st->d_vectors, artis_dep::NVECTORS * nn, down));
  HIP_TRY(stage_copy(out->totmassnuclide, st->d_totmass, nn, down));
  HIP_TRY(stage_copy(out->totals, st->d_totals, artis_dep::NTOTALS, down));
  HIP_TRY(stage_copy(&out->mtot, st->d_totmass + nn, 1, down));
  out->npts_nonempty = (int32_t)n;
  out->nnuclides = (int32_t)nn;
  out->nradioactive = st->T.nrad;
  out->nts_next = st->nts_next;
  out->t_mid = st->t_mid;
  for (int k = 0; k < 3; k++) out->kernel_ms[k] = st->kernel_ms[k];
  return ARTIS_OK;
}

int artis_amd_deposition_devptr(artis_amd_engine *e, const double **eps_ana, const float **grey_depth, const int32_t **thick, int64_t *npts_nonempty) {
  if (!e) return stage_error(ARTIS_ERR_ARG, "deposition: null engine");
  if (!e->dep || !e->dep->valid) return stage_error(ARTIS_ERR_ARG, "deposition: nothing updated (artis_amd_deposition_update)");
  if (eps_ana) *eps_ana = e->dep->d_cell;
  if (grey_depth) *grey_depth = e->dep->d_grey;
  if (thick) *thick = e->dep->d_thick;
  if (npts_nonempty) *npts_nonempty = e->dep->ncell;
  return ARTIS_OK;
}

int artis_amd_grid_update_deposited(artis_amd_engine *e, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream) {
  if (!e || !u || !ts_next) return stage_error(ARTIS_ERR_ARG, "grid_update_deposited: null engine, update or timestep");
#ifdef ARTIS_PRESET_NLTENEBULAR
  return stage_error(ARTIS_ERR_UNSUPPORTED, "grid_update_deposited: this build has NLTE populations (the nebular family): the ion balance is the host's");
#endif
  STAGE_STRUCT_SIZE(u, artis_grid_update, "grid_update_deposited");
  if (!e->decay || !e->decay->valid) return stage_error(ARTIS_ERR_ARG, "grid_update_deposited: no decay update (artis_amd_decay_update)");
  if (e->decay->t_mid != ts_next->mid) return stage_error(ARTIS_ERR_ARG, "grid_update_deposited: the decay update was made for another t_mid than ts_next->mid");
  if (!e->dep || !e->dep->valid) return stage_error(ARTIS_ERR_ARG, "grid_update_deposited: no deposition update (artis_amd_deposition_update)");
  if (e->dep->decay_serial != e->decay->serial || e->dep->t_mid != ts_next->mid)
    return stage_error(ARTIS_ERR_ARG, "grid_update_deposited: the deposition update was not made on the decay update of ts_next->mid");
  if (e->dep->nts_next != ts_next->nts) return stage_error(ARTIS_ERR_ARG, "grid_update_deposited: the deposition update was made for another nts than ts_next->nts");
  if (u->rho || u->elem_massfracs || u->elem_meanweight || u->thick)
    return stage_error(ARTIS_ERR_ARG, "grid_update_deposited: rho, elem_massfracs, elem_meanweight and thick must be NULL (they are the decay and deposition updates')");
  const IbMatter matter{e->decay->d_rho, e->decay->d_massfrac, e->decay->d_meanweight, e->dep->d_thick};
  return ib_grid_update(e, u, ts_next, hip_stream, &matter);
}

}  // extern "C"
