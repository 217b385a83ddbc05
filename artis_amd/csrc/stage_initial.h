// stage_initial.h -- artis_amd_initial_state*: the cells' temperatures, grey opacity and thickness before the first timestep (rules and
// bodies: initial_state.h), and artis_amd_grid_update_initial, which hands them with the decay update's matter to the ion balance
// (stage_ionbal.h) as the engine's FIRST cell state, without the host and without a resident state.
// Kernels on the caller's stream, every output element with one writer and no float atomics: k_init_energy (one lane per decay path:
// its energy per mass of the top nuclide with the expansion factor, the chain's scale and x_dom; skipped when the host hands its vector
// in) and k_init_cells (one lane per cell, one wave per workgroup as k_pinit_checkpoints: ONE walk over the paths' X lines without a
// checkpoint store -- X is [nuclide][cell], so the wave's loads of one path are one 256-byte line; top[p] and E[p] are indexed by the
// loop counter only and stay wave-uniform; CKPT_DEPTH lines are in flight before the first dependent addition -- then T_initial,
// kappagrey, the grey depth and the flags of the same cell). The counts of the three clamped branches and of the invalid opacities
// are a ballot each and, where the ballot is not empty, one integer atomic per wave; the first non-finite cell is an integer atomicMin
// of the wave's lowest such lane (the cells inside the bounds are the rest).
#pragma once

namespace {

struct InitArgs {
  artis_pinit::Tables T;
  double tstart;
  const float *X;  // [nuclide][cell]
  int64_t ncell;
  double *E, *scale, *x_dom;  // [npaths]
  artis_init::CellIn in;
  artis_init::Grey G;
  artis_dep::Step S;
  artis_init::CellOut out;
  float *W;               // [cell] ones: the dilution factor of grid.cc:1133
  int32_t *thick_before;  // [cell] THICK: what update_grid.cc:495-501 takes every cell for while W == 1
  int32_t *counts;        // {below MINTEMP, above MAXTEMP, non-finite, invalid kappagrey, the first non-finite cell}
};
enum { INIT_NCOUNTS = 5, INIT_FIRST = 4 };

__global__ void __launch_bounds__(BLOCK) k_init_energy(InitArgs a) {
  const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (p < a.T.npaths) a.E[p] = artis_init::path_energy_expansion(a.T, (int)p, a.tstart, &a.scale[p], &a.x_dom[p]);
}

// one wave per workgroup. A lane past the last cell walks the last cell's lines (in bounds, no divergence in the loop) and stores nothing.
__global__ void __launch_bounds__(64) k_init_cells(InitArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool mine = c < a.ncell;
  const int64_t cc = mine ? c : a.ncell - 1;
  const double sum = artis_pinit::cell_checkpoints(a.T.npaths, a.T.path_top, a.E, a.X, a.ncell, cc, nullptr, false);
  int32_t flags = 0;
  if (mine) {  // (stores last: the table loads above stay scalar)
    flags = artis_init::cell_entry(sum, a.in, a.G, a.S, c, a.out);
    a.W[c] = 1.f;
    a.thick_before[c] = ARTIS_CELL_THICK;
  }
  const int lane = threadIdx.x;
  const int branch = flags & ARTIS_INITIAL_BRANCH_MASK;
  const unsigned long long below = __ballot(branch == ARTIS_INITIAL_BELOW_MINTEMP), above = __ballot(branch == ARTIS_INITIAL_ABOVE_MAXTEMP);
  const unsigned long long nonfinite = __ballot(branch == ARTIS_INITIAL_NONFINITE), badkappa = __ballot((flags & ARTIS_INITIAL_KAPPA_INVALID) != 0);
  if (lane == 0) {
    if (below) atomicAdd(&a.counts[0], __popcll(below));
    if (above) atomicAdd(&a.counts[1], __popcll(above));
    if (nonfinite) atomicAdd(&a.counts[2], __popcll(nonfinite));
    if (badkappa) atomicAdd(&a.counts[3], __popcll(badkappa));
  }
  if (nonfinite && lane == __ffsll((long long)nonfinite) - 1) atomicMin(&a.counts[INIT_FIRST], (int32_t)c);
}

// everything of artis_amd_initial_state*: one block, made at the first call (and again when the network's size has changed)
struct InitState {
  StageBlock *block = nullptr;
  int64_t ncell = 0, nions = 0;
  int32_t npaths = 0;
  double *d_E = nullptr, *d_scale = nullptr, *d_x_dom = nullptr, *d_endecay = nullptr;
  float *d_T = nullptr, *d_kappagrey = nullptr, *d_grey = nullptr, *d_W = nullptr, *d_ffegrp = nullptr, *d_ye = nullptr, *d_ground_before = nullptr;
  int32_t *d_thick = nullptr, *d_flags = nullptr, *d_thick_before = nullptr, *d_counts = nullptr;
  double tstart = 0.;
  int32_t nts_first = 0, grey_type = 0;
  uint64_t decay_serial = 0;  // the decay update this state was made on
  bool valid = false;
  int64_t ncells_branch[4] = {}, ncells_kappa_invalid = 0;
  int32_t first_nonfinite = -1;
  double first_rho_tmin = 0., first_endecay = 0.;
  double kernel_ms[2] = {};
  ~InitState() { delete block; }
};

void init_free(InitState *st) { delete st; }
void init_invalidate(InitState *st) {
  if (st) st->valid = false;
}

int init_block(artis_amd_engine *e, const int64_t n, const int np) {
  InitState *st = e->init;
  if (st && st->block && st->ncell == n && st->npaths == np) return ARTIS_OK;
  init_free(e->init);
  e->init = nullptr;
  st = new InitState();
  st->block = new StageBlock();
  st->ncell = n;
  st->npaths = np;
  st->nions = e->Mh.nions;
  std::vector<StagePiece> pieces{piece(&st->d_E, np), piece(&st->d_scale, np), piece(&st->d_x_dom, np), piece(&st->d_endecay, n)};
  for (float **p : {&st->d_T, &st->d_kappagrey, &st->d_grey, &st->d_W, &st->d_ffegrp, &st->d_ye}) pieces.push_back(piece(p, n));
  pieces.insert(pieces.end(), {piece(&st->d_ground_before, n * st->nions), piece(&st->d_thick, n), piece(&st->d_flags, n), piece(&st->d_thick_before, n),
                               piece(&st->d_counts, INIT_NCOUNTS)});
  const int rc = st->block->make(pieces, "initial_state", "the result block");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  e->init = st;
  return ARTIS_OK;
}

}  // namespace

extern "C" {

int artis_amd_initial_state(artis_amd_engine *e, const artis_initial_params *p, void *hip_stream) {
  if (!e || !p) return stage_error(ARTIS_ERR_ARG, "initial_state: null engine or parameters");
#ifdef ARTIS_PRESET_NLTENEBULAR
  return stage_error(ARTIS_ERR_UNSUPPORTED, "initial_state: this build has NLTE populations (the nebular family): the first cell state is the host's");
#endif
  STAGE_STRUCT_SIZE(p, artis_initial_params, "initial_state");
  if (!e->decay) return stage_error(ARTIS_ERR_ARG, "initial_state: no network (artis_amd_decay_setup)");
  if (!e->dep) return stage_error(ARTIS_ERR_ARG, "initial_state: no energies (artis_amd_deposition_setup)");
  if (!e->pinit) return stage_error(ARTIS_ERR_ARG, "initial_state: no pellet set-up (artis_amd_packet_init_setup)");
  const DecayState *dc = e->decay;
  const int64_t n = dc->ncell;
  const int np = dc->T.npaths;
  const std::string bad = artis_init::initial_validate(*p, n, dc->t_model);
  if (!bad.empty()) return stage_error(ARTIS_ERR_ARG, "initial_state: " + bad);
  if (!dc->valid || dc->t_mid != p->tstart)
    return stage_error(ARTIS_ERR_ARG, "initial_state: no decay update at t_mid == tstart (artis_amd_decay_update: its rho and elem_massfracs)");
  if (p->energy_vector) {
    const std::string badv = artis_pinit::energy_vector_validate(p->energy_vector, np);
    if (!badv.empty()) return stage_error(ARTIS_ERR_ARG, "initial_state: energy_vector: " + badv);
  }
  HIP_TRY(hipSetDevice(e->device));
  int rc = init_block(e, n, np);
  if (rc != ARTIS_OK) return rc;
  InitState *st = e->init;
  st->valid = false;
  hipStream_t s = (hipStream_t)hip_stream;
  const bool fegroup = p->rpkt_grey_type == ARTIS_GREY_FEGROUP_APPROX, tanaka = p->rpkt_grey_type == ARTIS_GREY_TANAKA2020;
  if (fegroup) HIP_TRY(stage_copy(st->d_ffegrp, p->ffegrp, n, hipMemcpyHostToDevice, &s));
  if (tanaka) HIP_TRY(stage_copy(st->d_ye, p->initelectronfrac, n, hipMemcpyHostToDevice, &s));
  const int32_t counts0[INIT_NCOUNTS] = {0, 0, 0, 0, 0x7fffffff};
  HIP_TRY(stage_copy(st->d_counts, counts0, INIT_NCOUNTS, hipMemcpyHostToDevice, &s));
  HIP_TRY(hipStreamSynchronize(s));  // (the caller's arrays and counts0 are free again)

  InitArgs a{};
  a.T = e->pinit->T;
  a.tstart = p->tstart;
  a.X = dc->d_X;
  a.ncell = n;
  a.E = st->d_E;
  a.scale = st->d_scale;
  a.x_dom = st->d_x_dom;
  a.in.rho_tmin = dc->d_rho_tmin;
  a.in.rho = dc->d_rho;
  a.in.massfrac = dc->d_massfrac;
  a.in.initenergyq = e->pinit->T.initenergyq;  // (null unless the pellet set-up has both switches: grid.cc:1106)
  a.in.radial_pos_tmin = e->dep->d_radial;
  a.in.tmin = e->model_copy.tmin;
  a.in.tstart = p->tstart;
  a.G.type = p->rpkt_grey_type;
  a.G.mfegroup = p->mfegroup;
  a.G.mtot_input = p->mtot_input;
  a.G.ffegrp = fegroup ? st->d_ffegrp : nullptr;
  a.G.initelectronfrac = tanaka ? st->d_ye : nullptr;
  a.G.elem_anumber = e->M.elem_anumber;
  a.G.nelements = e->Mh.nelements;
  a.S.t_mid = p->tstart;
  a.S.tmin = e->model_copy.tmin;
  a.S.rmax = e->model_copy.rmax;
  a.S.nts_next = p->nts_first;
  a.S.num_grey_timesteps = p->num_grey_timesteps;
  a.S.optical_depth_is_thick = p->optical_depth_is_thick;
  a.S.optical_depth_is_thick_vpkt = p->optical_depth_is_thick_vpkt;
  a.out.T_initial = st->d_T;
  a.out.kappagrey = st->d_kappagrey;
  a.out.grey_depth = st->d_grey;
  a.out.endecay = st->d_endecay;
  a.out.thick = st->d_thick;
  a.out.flags = st->d_flags;
  a.W = st->d_W;
  a.thick_before = st->d_thick_before;
  a.counts = st->d_counts;
  auto done = [&](const char *kernel) -> int {
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("initial_state: ") + kernel + ": " + hipGetErrorString(err));
    return ARTIS_OK;
  };
  HIP_TRY(hipEventRecord(st->block->ev[0], s));
  if (p->energy_vector) {
    HIP_TRY(stage_copy(st->d_E, p->energy_vector, np, hipMemcpyHostToDevice, &s));
    if (np > 0) {
      HIP_TRY(hipMemsetAsync(st->d_scale, 0, sizeof(double) * (size_t)np, s));
      HIP_TRY(hipMemsetAsync(st->d_x_dom, 0, sizeof(double) * (size_t)np, s));
    }
    HIP_TRY(hipStreamSynchronize(s));  // (the caller's array is free again)
  } else if (np > 0) {
    hipLaunchKernelGGL(k_init_energy, dim3(nblocks(np)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_init_energy")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block->ev[1], s));
  if (n > 0) {
    hipLaunchKernelGGL(k_init_cells, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a);
    if ((rc = done("k_init_cells")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block->ev[2], s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 2; k++) HIP_TRY(st->block->elapsed_ms(k, &st->kernel_ms[k]));
  int32_t counts[INIT_NCOUNTS] = {};
  HIP_TRY(stage_copy(counts, st->d_counts, INIT_NCOUNTS, hipMemcpyDeviceToHost));
  st->ncells_branch[ARTIS_INITIAL_BELOW_MINTEMP] = counts[0];
  st->ncells_branch[ARTIS_INITIAL_ABOVE_MAXTEMP] = counts[1];
  st->ncells_branch[ARTIS_INITIAL_NONFINITE] = counts[2];
  st->ncells_branch[ARTIS_INITIAL_INSIDE] = n - counts[0] - counts[1] - counts[2];
  st->ncells_kappa_invalid = counts[3];
  st->first_nonfinite = counts[2] > 0 ? counts[INIT_FIRST] : -1;
  st->first_rho_tmin = st->first_endecay = 0.;
  if (st->first_nonfinite >= 0 && st->first_nonfinite < n) {
    float rho_tmin = 0.f;
    HIP_TRY(stage_copy(&rho_tmin, dc->d_rho_tmin + st->first_nonfinite, 1, hipMemcpyDeviceToHost));
    HIP_TRY(stage_copy(&st->first_endecay, st->d_endecay + st->first_nonfinite, 1, hipMemcpyDeviceToHost));
    st->first_rho_tmin = rho_tmin;
  }
  st->tstart = p->tstart;
  st->nts_first = p->nts_first;
  st->grey_type = p->rpkt_grey_type;
  st->decay_serial = dc->serial;
  st->valid = true;
  return ARTIS_OK;
}

int artis_amd_initial_state_download(artis_amd_engine *e, artis_initial_result *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "initial_state: null argument");
  STAGE_STRUCT_SIZE(out, artis_initial_result, "initial_state");
  if (!e->init || !e->init->valid) return stage_error(ARTIS_ERR_ARG, "initial_state: nothing made (artis_amd_initial_state)");
  InitState *st = e->init;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell, np = st->npaths;
  const hipMemcpyKind down = hipMemcpyDeviceToHost;
  HIP_TRY(stage_copy(out->T_initial, st->d_T, n, down));
  HIP_TRY(stage_copy(out->endecay_per_mass, st->d_endecay, n, down));
  HIP_TRY(stage_copy(out->kappagrey, st->d_kappagrey, n, down));
  HIP_TRY(stage_copy(out->grey_depth, st->d_grey, n, down));
  HIP_TRY(stage_copy(out->thick, st->d_thick, n, down));
  HIP_TRY(stage_copy(out->flags, st->d_flags, n, down));
  HIP_TRY(stage_copy(out->energy_vector, st->d_E, np, down));
  HIP_TRY(stage_copy(out->path_scale, st->d_scale, np, down));
  HIP_TRY(stage_copy(out->path_x_dom, st->d_x_dom, np, down));
  for (int k = 0; k < 4; k++) out->ncells_branch[k] = st->ncells_branch[k];
  out->ncells_kappa_invalid = st->ncells_kappa_invalid;
  out->first_nonfinite_cell = st->first_nonfinite;
  out->npts_nonempty = (int32_t)n;
  out->npaths = (int32_t)np;
  out->rpkt_grey_type = st->grey_type;
  out->nts_first = st->nts_first;
  out->reserved = 0;
  out->first_nonfinite_rho_tmin = st->first_rho_tmin;
  out->first_nonfinite_endecay = st->first_endecay;
  out->tstart = st->tstart;
  for (int k = 0; k < 2; k++) out->kernel_ms[k] = st->kernel_ms[k];
  return ARTIS_OK;
}

int artis_amd_grid_update_initial(artis_amd_engine *e, const artis_grid_update *u, const artis_timestep *ts_first, void *hip_stream) {
  if (!e || !u || !ts_first) return stage_error(ARTIS_ERR_ARG, "grid_update_initial: null engine, update or timestep");
#ifdef ARTIS_PRESET_NLTENEBULAR
  return stage_error(ARTIS_ERR_UNSUPPORTED, "grid_update_initial: this build has NLTE populations (the nebular family): the ion balance is the host's");
#endif
  STAGE_STRUCT_SIZE(u, artis_grid_update, "grid_update_initial");
  if (!e->init || !e->init->valid) return stage_error(ARTIS_ERR_ARG, "grid_update_initial: no initial state (artis_amd_initial_state)");
  if (!e->decay || !e->decay->valid) return stage_error(ARTIS_ERR_ARG, "grid_update_initial: no decay update (artis_amd_decay_update)");
  const InitState *st = e->init;
  if (e->decay->t_mid != ts_first->mid || st->decay_serial != e->decay->serial || st->tstart != ts_first->mid)
    return stage_error(ARTIS_ERR_ARG, "grid_update_initial: the initial state was not made on the decay update of ts_first->mid");
  if (st->nts_first != ts_first->nts) return stage_error(ARTIS_ERR_ARG, "grid_update_initial: the initial state was made for another nts than ts_first->nts");
  if (u->use_fit != 0) return stage_error(ARTIS_ERR_ARG, "grid_update_initial: use_fit must be 0 (the first timestep has no fit)");
  if (u->TJ || u->TR || u->W || u->Te || u->rho || u->elem_massfracs || u->elem_meanweight || u->thick || u->kappagrey)
    return stage_error(ARTIS_ERR_ARG, "grid_update_initial: TJ, TR, W, Te, rho, elem_massfracs, elem_meanweight, thick and kappagrey must be NULL (they are the "
                                      "initial state's and the decay update's)");
  if (!e->have_cells && !u->clumpfactor) return stage_error(ARTIS_ERR_ARG, "grid_update_initial: clumpfactor is required while no cell state is resident");
  if (st->ncells_kappa_invalid > 0)
    return stage_error(ARTIS_ERR_ARG, "grid_update_initial: " + std::to_string(st->ncells_kappa_invalid) + " cells with a negative or non-finite kappagrey");
  IbMatter matter{e->decay->d_rho, e->decay->d_massfrac, e->decay->d_meanweight, st->d_thick};
  matter.initial_T = st->d_T;
  matter.initial_W = st->d_W;
  matter.initial_kappagrey = st->d_kappagrey;
  matter.initial_ground = st->d_ground_before;
  matter.initial_thick = st->d_thick_before;
  return ib_grid_update(e, u, ts_first, hip_stream, &matter);
}

}  // extern "C"
