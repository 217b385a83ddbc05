// stage_ionbal.h -- artis_amd_grid_update*: the ionisation balance and the hand-over to the cell state (rules and per-element
// bodies: ion_balance.h).
// Kernels on the caller's stream, every output element with one writer: k_ib_alpha_sp (first call: the [nions][TABLESIZE]
// ion_alpha_sp table and each ion's ground-continuum index), k_ib_cells (one lane per cell: temperatures, nnetot), k_ib_gamma (one
// lane per (cell, ground continuum): the normalised gamma estimator), k_ib_partfunct (one lane per (cell, ion), levels summed in
// order), k_ib_phi (one lane per (cell, ion): phi once, into a [cell][ion] array), k_ib_solve (one lane per cell: uppermost ions,
// n_e root search, ground populations, final n_e). Flags are integer ORs. Nothing reaches the engine's cell state until every
// cell has been balanced; then the arrays are copied over and the cell cache is filled.
#pragma once

namespace {

struct IbArgs {
  artis::DevModel M;
  int64_t ncell;
  int32_t use_fit, lte;
  // inputs
  const float *fit_TJ, *fit_TR, *fit_W, *fit_Te;  // the fit's (use_fit) or the host's (uploaded)
  const int32_t *fit_flags;                       // the fit's per-cell flags (use_fit), else null
  const float *host_Te;                           // Te override of fitted cells, or null
  const float *cur_ground;                        // the cell state's ground populations (for the partition functions)
  const int32_t *cur_thick;                       // ... thickness (the balance's Saha switch)
  const double *gamma_raw;                        // [cell][ground continuum][2]{gamma, bfheating} of the estimator block
  const double *assocvol;
  double prev_mid, tmin, deltat;
  int32_t nprocs;
  const float *clump;
  // scratch / outputs: the arrays of the set-up and the solve (cell), and what the kernels before the solve write
  artis_ib::CellArrays cell;
  float *alpha_sp;
  int32_t *gci;
  float *TJ, *TR, *W, *Te, *nnetot, *U;
  double *gamma, *phi;
};

__global__ void __launch_bounds__(BLOCK) k_ib_alpha_sp(IbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (int64_t)a.M.nions * ARTIS_OPT_TABLESIZE) return;
  const int ui = (int)(i / ARTIS_OPT_TABLESIZE);
  artis_ib::alpha_sp_entry(a.M, ui, (int)(i - (int64_t)ui * ARTIS_OPT_TABLESIZE), a.alpha_sp, a.gci);
}

__global__ void __launch_bounds__(BLOCK) k_ib_cells(IbArgs a) {
  const int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (c >= a.ncell) return;
  artis_ib::cell_setup(a.M, c, a.cell, a.fit_Te, a.host_Te, a.fit_flags, artis_ib::cell_forced_saha(a.lte, a.cur_thick[c]), a.Te, a.nnetot);
  a.TJ[c] = a.fit_TJ[c];  // (the radiation temperatures pass through)
  a.TR[c] = a.fit_TR[c];
  a.W[c] = a.fit_W[c];
}

__global__ void __launch_bounds__(BLOCK) k_ib_gamma(IbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.ncell * a.cell.nbfg) return;
  a.gamma[i] = a.use_fit ? artis_ib::gamma_normed_entry(a.gamma_raw[2 * i], a.assocvol[i / a.cell.nbfg], a.prev_mid, a.tmin, a.deltat, a.nprocs)
                         : 0.;
}

__global__ void __launch_bounds__(BLOCK) k_ib_partfunct(IbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.ncell * a.M.nions) return;
  const int64_t c = i / a.M.nions;
  int32_t flags = 0;
  artis_ib::partfunct_entry(a.M, c, (int)(i - c * a.M.nions), a.TJ, a.Te, a.cur_ground, a.cell.massfrac, a.U, &flags);
  if (flags) atomicOr(&a.cell.flags[c], flags);
}

__global__ void __launch_bounds__(BLOCK) k_ib_phi(IbArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.ncell * a.M.nions) return;
  const int64_t c = i / a.M.nions;
  artis_ib::phi_entry(a.M, c, (int)(i - c * a.M.nions), a.cell.flags[c], a.U, a.Te, a.clump, a.alpha_sp, a.gci, a.gamma, a.cell.nbfg, a.phi);
}

__global__ void __launch_bounds__(BLOCK) k_ib_solve(IbArgs a) {
  const int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (c >= a.ncell) return;
  artis_ib::solve_cell(a.M, c, a.cell);
}

// corrphotoionrenorm = 1 in the cells balanced with forced Saha (update_grid.cc:539-543)
__global__ void __launch_bounds__(BLOCK) k_ib_renorm(double *renorm, const int32_t *flags, int64_t ncell, int32_t nbfg) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= ncell * nbfg) return;
  if (flags[i / nbfg] & artis_ib::FORCED_SAHA) renorm[i] = 1.;
}

// dst[cell][ground continuum] = src[...] in the cells the fit has fitted (artis_amd_grid_update_thermal)
__global__ void __launch_bounds__(BLOCK) k_ib_fitted_copy(double *dst, const double *src, const int32_t *fit_flags, int64_t ncell, int32_t nbfg) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= ncell * nbfg) return;
  if (fit_flags[i / nbfg] & ARTIS_RADFIELD_FITTED) dst[i] = src[i];
}

// the scratch of artis_amd_grid_update*: one block, made at the first call
struct IbState {
  StageBlock block;
  int64_t ncell = 0, nions = 0, nelements = 0, nbfg = 0;
  float *d_alpha_sp = nullptr, *d_hTJ = nullptr, *d_hTR = nullptr, *d_hW = nullptr, *d_hTe = nullptr;
  int32_t *d_gci = nullptr, *d_thick = nullptr;
  float *d_rho = nullptr, *d_massfrac = nullptr, *d_meanweight = nullptr, *d_kappagrey = nullptr, *d_clump = nullptr, *d_ffegrp = nullptr;
  float *d_TJ = nullptr, *d_TR = nullptr, *d_W = nullptr, *d_Te = nullptr, *d_nnetot = nullptr, *d_U = nullptr, *d_ground = nullptr;
  float *d_nne = nullptr, *d_nne_root = nullptr;
  double *d_gamma = nullptr, *d_phi = nullptr;
  int32_t *d_uppermost = nullptr, *d_flags = nullptr, *d_evals = nullptr;
  bool have_alpha_sp = false, valid = false;
  int64_t ncells_flagged[8] = {}, total_evals = 0;
  double kernel_ms[ARTIS_IONBAL_NTIMES] = {};
};

void ib_free(IbState *st) { delete st; }

int ib_init(artis_amd_engine *e) {
  if (e->ib) return ARTIS_OK;
  const DevModel &h = e->Mh;
  // the per-cell solve holds one element's ion fractions in registers / scratch of MAXIONS entries
  std::vector<int32_t> nions((size_t)(h.nelements > 0 ? h.nelements : 1));
  if (h.nelements > 0)
    HIP_TRY(hipMemcpy(nions.data(), e->M.elem_nions, sizeof(int32_t) * (size_t)h.nelements, hipMemcpyDeviceToHost));
  for (int el = 0; el < h.nelements; el++)
    if (nions[(size_t)el] > artis_ib::MAXIONS)
      return stage_error(ARTIS_ERR_UNSUPPORTED, "grid_update: an element has more than " + std::to_string(artis_ib::MAXIONS) + " ions");
  IbState *st = new IbState();
  const int64_t n = st->ncell = h.npts_nonempty, ni = st->nions = h.nions, ne = st->nelements = h.nelements;
  st->nbfg = h.nbfcontinua_ground;
  std::vector<StagePiece> pieces{piece(&st->d_alpha_sp, ni * ARTIS_OPT_TABLESIZE), piece(&st->d_gci, ni)};
  for (float **p : {&st->d_hTJ, &st->d_hTR, &st->d_hW, &st->d_hTe, &st->d_rho, &st->d_kappagrey, &st->d_clump, &st->d_ffegrp, &st->d_TJ,
                    &st->d_TR, &st->d_W, &st->d_Te, &st->d_nnetot, &st->d_nne, &st->d_nne_root})
    pieces.push_back(piece(p, n));
  pieces.insert(pieces.end(), {piece(&st->d_thick, n), piece(&st->d_massfrac, n * ne), piece(&st->d_meanweight, n * ne), piece(&st->d_U, n * ni),
                               piece(&st->d_ground, n * ni), piece(&st->d_gamma, n * st->nbfg), piece(&st->d_phi, n * ni),
                               piece(&st->d_uppermost, n * ne), piece(&st->d_flags, n), piece(&st->d_evals, n)});
  const int rc = st->block.make(pieces, "grid_update", "the scratch");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  e->ib = st;
  return ARTIS_OK;
}

// where the new timestep's matter comes from when not from the host: device arrays (artis_amd_grid_update_decayed, stage_decay.h), and
// with them the next step's thickness flags (artis_amd_grid_update_deposited, stage_deposition.h; null: the host's u->thick)
struct IbMatter {
  const float *rho, *massfrac, *meanweight;
  const int32_t *thick = nullptr;
  // artis_amd_grid_update_thermal (stage_thermal.h): in the cells the fit has fitted, T_e, the balance's gamma [cell][ground continuum]
  // and the cell state's corrphotoionrenorm are the thermal solve's (device arrays)
  const float *thermal_Te = nullptr;
  const double *thermal_gamma = nullptr, *thermal_renorm = nullptr;
  const float *thermal_clump = nullptr;  // ... and the clumping factors of every cell the solve's (they become the cell state's)
  // artis_amd_grid_update_initial (stage_initial.h): the first timestep. T_J = T_R = T_e = initial_T, W = initial_W (ones) and
  // kappagrey are the initial state's (device arrays), and so is the balance's "current" state: ground populations of 0 and THICK
  // flags, what the reference holds before its first update_grid. No cell state has to be resident
  const float *initial_T = nullptr, *initial_W = nullptr, *initial_kappagrey = nullptr, *initial_ground = nullptr;
  const int32_t *initial_thick = nullptr;
};

__global__ void __launch_bounds__(BLOCK) k_ib_fill(double *dst, double value, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < count) dst[i] = value;
}

// The first cell state of an engine that has none (the hand-over of artis_amd_grid_update_initial): the arrays of
// artis_amd_set_cellstate, allocated zeroed, and what the hand-over below does not write. Where every array of DevCells that a
// supported build's propagation or a later stage reads then comes from:
//   rho, elem_massfracs, elem_meanweight (allocated here, ahead of the    the decay update, through the balance's scratch
//   options' refusals, in USE_CALCULATED_MEANATOMICWEIGHT builds)
//   Te, TJ, TR, W, kappagrey, thick                                       the initial state (stage_initial.h), through the scratch
//   nne, nnetot, ion_partfuncts, ion_groundlevelpops                      the balance
//   clumpfactor                                                           u->clumpfactor (required here)
//   ffegrp                                                                u->ffegrp, else zeros as artis_amd_set_cellstate uploads for an absent one
//   corrphotoionrenorm                                                    1 in every cell (grid.cc:561; the balance's forced Saha writes the same)
//   expansionopacities, expansionopacity_planck_cumulative                the engine's own, made at cell-cache population (cellstate_options)
//   levelpops, corrphotoioncoeff, radfieldbin_*, nt_*, Jb_lu_normed       absent, as after an artis_amd_set_cellstate without them; a build
//                                                                         that needs one from the host is refused by cellstate_options
// On an error no state is resident and nothing of it is kept.
int ib_first_cellstate(artis_amd_engine *e, hipStream_t s) {
  int rc = cellstate_alloc(e, true);
  const int64_t nmw = (int64_t)e->Mh.npts_nonempty * e->Mh.nelements;
  if (rc == ARTIS_OK && ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && nmw > 0) {
    // before cellstate_options: a build that reads element number densities (XCOM, NT_ON) refuses a state without this array
    float *d = nullptr;
    if (hipMalloc((void **)&d, sizeof(float) * (size_t)nmw) != hipSuccess) {
      rc = stage_error(ARTIS_ERR_HIP, "grid_update_initial: allocation of elem_meanweight");
    } else {
      e->cell_allocs.push_back(d);
      e->C.elem_meanweight = d;
    }
  }
  if (rc == ARTIS_OK) rc = cellstate_options(e, false);
  const int64_t nrenorm = (int64_t)e->Mh.npts_nonempty * (e->Mh.nbfcontinua_ground > 0 ? e->Mh.nbfcontinua_ground : 1);
  if (rc == ARTIS_OK && nrenorm > 0) {  // (after the allocation's hipMemset, which has ended when it returns: StageBlock::make relies on the same)
    hipLaunchKernelGGL(k_ib_fill, dim3(nblocks(nrenorm)), dim3(BLOCK), 0, s, const_cast<double *>(e->C.corrphotoionrenorm), 1., nrenorm);
    if (hipGetLastError() != hipSuccess) rc = stage_error(ARTIS_ERR_HIP, "grid_update_initial: k_ib_fill");
  }
  if (rc != ARTIS_OK) {
    free_all(e->cell_allocs);
    e->C = DevCells{};
  }
  return rc;
}

// artis_amd_grid_update (matter == nullptr: u's host arrays) and artis_amd_grid_update_decayed (matter: copied device to device into the same scratch)
int ib_grid_update(artis_amd_engine *e, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream, const IbMatter *matter) {
  if (!e || !u || !ts_next) return stage_error(ARTIS_ERR_ARG, "grid_update: null engine, update or timestep");
#ifdef ARTIS_PRESET_NLTENEBULAR
  return stage_error(ARTIS_ERR_UNSUPPORTED, "grid_update: this build has NLTE populations (the nebular family): the ion balance is the host's");
#endif
  STAGE_STRUCT_SIZE(u, artis_grid_update, "grid_update");
  const bool initial = matter && matter->initial_T;
  if (!e->have_cells && !initial) return stage_error(ARTIS_ERR_ARG, "grid_update: no cell state (artis_amd_set_cellstate)");
  if (u->use_fit != 0 && u->use_fit != 1) return stage_error(ARTIS_ERR_ARG, "grid_update: use_fit must be 0 or 1");
  if (u->use_fit && (!e->rf || !e->rf->valid || !e->fit_since_step))
    return stage_error(ARTIS_ERR_ARG, "grid_update: use_fit = 1 needs an artis_amd_radfield_fit since the last propagation call");
  if (!u->use_fit && !initial && (!u->TJ || !u->TR || !u->W || !u->Te)) return stage_error(ARTIS_ERR_ARG, "grid_update: use_fit = 0 needs TJ, TR, W and Te");
  if (!matter && (!u->rho || !u->elem_massfracs || !u->thick)) return stage_error(ARTIS_ERR_ARG, "grid_update: rho, elem_massfracs and thick are required");
  if (matter && !matter->thick && !u->thick) return stage_error(ARTIS_ERR_ARG, "grid_update: thick is required");
  if (!matter && ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && !u->elem_meanweight)
    return stage_error(ARTIS_ERR_ARG, "grid_update: this build has USE_CALCULATED_MEANATOMICWEIGHT: elem_meanweight is required");
  if (!ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && !e->M.elem_meannucmass)
    return stage_error(ARTIS_ERR_ARG, "grid_update: the element number densities need artis_model.elem_meannucmass");
  HIP_TRY(hipSetDevice(e->device));
  int rc = ib_init(e);
  if (rc != ARTIS_OK) return rc;
  IbState *st = e->ib;
  st->valid = false;
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t n = st->ncell, ni = st->nions, ne = st->nelements;
  const hipMemcpyKind from_matter = matter ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIP_TRY(stage_copy(st->d_rho, matter ? matter->rho : u->rho, n, from_matter, &s));
  HIP_TRY(stage_copy(st->d_massfrac, matter ? matter->massfrac : u->elem_massfracs, n * ne, from_matter, &s));
  if (matter && matter->thick)
    HIP_TRY(stage_copy(st->d_thick, matter->thick, n, hipMemcpyDeviceToDevice, &s));
  else
    HIP_TRY(stage_copy(st->d_thick, u->thick, n, hipMemcpyHostToDevice, &s));
  if (ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT)
    HIP_TRY(stage_copy(st->d_meanweight, matter ? matter->meanweight : u->elem_meanweight, n * ne, from_matter, &s));
  if (initial)
    HIP_TRY(stage_copy(st->d_kappagrey, matter->initial_kappagrey, n, hipMemcpyDeviceToDevice, &s));
  else
    HIP_TRY(stage_copy(st->d_kappagrey, u->kappagrey, n, hipMemcpyHostToDevice, &s));
  HIP_TRY(stage_copy(st->d_clump, u->clumpfactor, n, hipMemcpyHostToDevice, &s));
  HIP_TRY(stage_copy(st->d_ffegrp, u->ffegrp, n, hipMemcpyHostToDevice, &s));
  if (!u->use_fit && !initial) {
    HIP_TRY(stage_copy(st->d_hTJ, u->TJ, n, hipMemcpyHostToDevice, &s));
    HIP_TRY(stage_copy(st->d_hTR, u->TR, n, hipMemcpyHostToDevice, &s));
    HIP_TRY(stage_copy(st->d_hW, u->W, n, hipMemcpyHostToDevice, &s));
  }
  if (u->Te) HIP_TRY(stage_copy(st->d_hTe, u->Te, n, hipMemcpyHostToDevice, &s));
  IbArgs a{};
  a.M = e->M;
  a.ncell = n;
  a.use_fit = u->use_fit;
  a.lte = u->use_fit ? e->rf->lte : 1;
  a.fit_TJ = u->use_fit ? e->rf->d_TJ : st->d_hTJ;
  a.fit_TR = u->use_fit ? e->rf->d_TR : st->d_hTR;
  a.fit_W = u->use_fit ? e->rf->d_W : st->d_hW;
  a.fit_Te = u->use_fit ? e->rf->d_Te : st->d_hTe;
  a.fit_flags = u->use_fit ? e->rf->d_flags : nullptr;
  if (initial) {
    a.fit_TJ = a.fit_TR = a.fit_Te = matter->initial_T;
    a.fit_W = matter->initial_W;
  }
  a.host_Te = (u->use_fit && u->Te) ? st->d_hTe : nullptr;
  if (matter && matter->thermal_Te) a.host_Te = matter->thermal_Te;
  a.cur_ground = initial ? matter->initial_ground : e->C.ion_groundlevelpops;
  a.cur_thick = initial ? matter->initial_thick : e->C.thick;
  a.gamma_raw = e->E.gammaestimator;
  if (u->use_fit) {
    a.assocvol = e->rf->d_assocvol;
    a.prev_mid = e->rf->prev_mid;
    a.deltat = e->rf->deltat;
    a.nprocs = e->rf->nprocs;
  }
  a.tmin = e->model_copy.tmin;
  a.clump = u->clumpfactor ? st->d_clump : e->C.clumpfactor;
  if (matter && matter->thermal_clump) a.clump = matter->thermal_clump;
  a.cell.rho = st->d_rho;
  a.cell.massfrac = st->d_massfrac;
  a.cell.meanweight_cell = ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT ? st->d_meanweight : nullptr;
  a.cell.meanweight_model = e->M.elem_meannucmass;
  a.cell.U = a.U = st->d_U;
  a.cell.phi = a.phi = st->d_phi;
  a.cell.gamma = a.gamma = st->d_gamma;
  a.cell.gci = a.gci = st->d_gci;
  a.cell.nbfg = (int32_t)st->nbfg;
  a.cell.uppermost = st->d_uppermost;
  a.cell.flags = st->d_flags;
  a.cell.evals = st->d_evals;
  a.cell.ground = st->d_ground;
  a.cell.nne = st->d_nne;
  a.cell.nne_root = st->d_nne_root;
  a.alpha_sp = st->d_alpha_sp;
  a.TJ = st->d_TJ;
  a.TR = st->d_TR;
  a.W = st->d_W;
  a.Te = st->d_Te;
  a.nnetot = st->d_nnetot;
  // every kernel is checked where it ends, so that an error names it (the calls are few and the kernels short)
  auto done = [&](const char *kernel) -> int {
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("grid_update: ") + kernel + ": " + hipGetErrorString(err));
    return ARTIS_OK;
  };
  if (!st->have_alpha_sp && ni > 0) {  // kept for the engine's lifetime
    hipLaunchKernelGGL(k_ib_alpha_sp, dim3(nblocks(ni * ARTIS_OPT_TABLESIZE)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_ib_alpha_sp")) != ARTIS_OK) return rc;
    st->have_alpha_sp = true;
  }
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  if (n > 0) {
    hipLaunchKernelGGL(k_ib_cells, dim3(nblocks(n)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_ib_cells")) != ARTIS_OK) return rc;
    if (st->nbfg > 0) hipLaunchKernelGGL(k_ib_gamma, dim3(nblocks(n * st->nbfg)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_ib_gamma")) != ARTIS_OK) return rc;
    if (matter && matter->thermal_gamma && st->nbfg > 0) {
      hipLaunchKernelGGL(k_ib_fitted_copy, dim3(nblocks(n * st->nbfg)), dim3(BLOCK), 0, s, st->d_gamma, matter->thermal_gamma, a.fit_flags, n, (int32_t)st->nbfg);
      if ((rc = done("k_ib_fitted_copy")) != ARTIS_OK) return rc;
    }
    if (ni > 0) hipLaunchKernelGGL(k_ib_partfunct, dim3(nblocks(n * ni)), dim3(BLOCK), 0, s, a);
    if ((rc = done("k_ib_partfunct")) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[1], s));
  if (n > 0 && ni > 0) hipLaunchKernelGGL(k_ib_phi, dim3(nblocks(n * ni)), dim3(BLOCK), 0, s, a);
  if ((rc = done("k_ib_phi")) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->block.ev[2], s));
  if (n > 0) hipLaunchKernelGGL(k_ib_solve, dim3(nblocks(n)), dim3(BLOCK), 0, s, a);
  if ((rc = done("k_ib_solve")) != ARTIS_OK) return rc;
  HIP_TRY(hipEventRecord(st->block.ev[3], s));
  std::vector<int32_t> flags((size_t)n), evals((size_t)n);
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(flags.data(), st->d_flags, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(evals.data(), st->d_evals, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) HIP_TRY(st->block.elapsed_ms(k, &st->kernel_ms[k]));
  st->kernel_ms[3] = 0.;
  int64_t refused = 0;
  std::fill(std::begin(st->ncells_flagged), std::end(st->ncells_flagged), 0);
  st->total_evals = 0;
  for (int64_t c = 0; c < n; c++) {
    for (int k = 0; k < 8; k++)
      if (flags[(size_t)c] & (1 << k)) st->ncells_flagged[k]++;
    if (flags[(size_t)c] & artis_ib::REFUSED) refused++;
    st->total_evals += evals[(size_t)c];
  }
  st->valid = true;
  if (refused > 0)
    return stage_error(ARTIS_ERR_NOTCONVERGED, "grid_update: " + std::to_string(refused) + " cells unbracketed, non-finite or with an invalid partition function (" +
                                                std::to_string(st->ncells_flagged[4]) + " / " + std::to_string(st->ncells_flagged[6]) + " / " +
                                                std::to_string(st->ncells_flagged[5]) + "); the previous cell state stays");
  // the hand-over: the engine's cell state becomes the result (artis_amd_set_cellstate), then the cell cache is filled
  const bool first_state = !e->have_cells;
  if (first_state && (rc = ib_first_cellstate(e, s)) != ARTIS_OK) return rc;
  if (ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && !e->C.elem_meanweight && n * ne > 0) {
    float *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, sizeof(float) * (size_t)(n * ne)));
    e->cell_allocs.push_back(d);
    e->C.elem_meanweight = d;
  }
  HIP_TRY(stage_copy(e->C.rho, st->d_rho, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.Te, st->d_Te, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.TJ, st->d_TJ, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.TR, st->d_TR, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.W, st->d_W, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.nne, st->d_nne, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.nnetot, st->d_nnetot, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.ion_partfuncts, st->d_U, n * ni, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.ion_groundlevelpops, st->d_ground, n * ni, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(stage_copy(e->C.elem_massfracs, st->d_massfrac, n * ne, hipMemcpyDeviceToDevice, &s));
  if (ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT) HIP_TRY(stage_copy(e->C.elem_meanweight, st->d_meanweight, n * ne, hipMemcpyDeviceToDevice, &s));
  if (u->kappagrey || initial) HIP_TRY(stage_copy(e->C.kappagrey, st->d_kappagrey, n, hipMemcpyDeviceToDevice, &s));
  if (u->clumpfactor) HIP_TRY(stage_copy(e->C.clumpfactor, st->d_clump, n, hipMemcpyDeviceToDevice, &s));
  if (matter && matter->thermal_clump) HIP_TRY(stage_copy(e->C.clumpfactor, matter->thermal_clump, n, hipMemcpyDeviceToDevice, &s));
  if (u->ffegrp) HIP_TRY(stage_copy(e->C.ffegrp, st->d_ffegrp, n, hipMemcpyDeviceToDevice, &s));
  if (ARTIS_OPT_USE_LUT_PHOTOION && n > 0 && st->nbfg > 0) {
    hipLaunchKernelGGL(k_ib_renorm, dim3(nblocks(n * st->nbfg)), dim3(BLOCK), 0, s, const_cast<double *>(e->C.corrphotoionrenorm),
                       st->d_flags, n, (int32_t)st->nbfg);
    HIP_TRY(hipGetLastError());
    if (matter && matter->thermal_renorm) {
      hipLaunchKernelGGL(k_ib_fitted_copy, dim3(nblocks(n * st->nbfg)), dim3(BLOCK), 0, s, const_cast<double *>(e->C.corrphotoionrenorm),
                         matter->thermal_renorm, a.fit_flags, n, (int32_t)st->nbfg);
      HIP_TRY(hipGetLastError());
    }
  }
  // (the thickness last: the balance and the renormalisation read the current one)
  HIP_TRY(stage_copy(e->C.thick, st->d_thick, n, hipMemcpyDeviceToDevice, &s));
  HIP_TRY(hipStreamSynchronize(s));
  e->have_cells = true;  // (it was, but after the first state of artis_amd_grid_update_initial)
  e->cellstate_serial++;
  e->S = make_step(*ts_next);
  const auto t0 = std::chrono::steady_clock::now();
  rc = artis_amd_populate_cellcache(e, hip_stream);
  st->kernel_ms[3] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

}  // namespace

extern "C" {

int artis_amd_grid_update(artis_amd_engine *e, const artis_grid_update *u, const artis_timestep *ts_next, void *hip_stream) {
  return ib_grid_update(e, u, ts_next, hip_stream, nullptr);
}

int artis_amd_grid_update_download(artis_amd_engine *e, artis_grid_update_result *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "grid_update: null argument");
  STAGE_STRUCT_SIZE(out, artis_grid_update_result, "grid_update");
  if (!e->ib || !e->ib->valid) return stage_error(ARTIS_ERR_ARG, "grid_update: nothing balanced (artis_amd_grid_update)");
  IbState *st = e->ib;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell, ni = st->nions, ne = st->nelements;
  HIP_TRY(stage_copy(out->Te, st->d_Te, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->TJ, st->d_TJ, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->TR, st->d_TR, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->W, st->d_W, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->nne, st->d_nne, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->nnetot, st->d_nnetot, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->rho, st->d_rho, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->ion_partfuncts, st->d_U, n * ni, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->ion_groundlevelpops, st->d_ground, n * ni, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->uppermost_ion, st->d_uppermost, n * ne, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->gamma_normed, st->d_gamma, n * st->nbfg, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->phi, st->d_phi, n * ni, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->nne_root, st->d_nne_root, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->flags, st->d_flags, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->evals, st->d_evals, n, hipMemcpyDeviceToHost));
  for (int k = 0; k < 8; k++) out->ncells_flagged[k] = st->ncells_flagged[k];
  out->total_evals = st->total_evals;
  out->npts_nonempty = (int32_t)n;
  out->nions = (int32_t)ni;
  out->nelements = (int32_t)ne;
  out->nbfcontinua_ground = (int32_t)st->nbfg;
  for (int k = 0; k < ARTIS_IONBAL_NTIMES; k++) out->kernel_ms[k] = st->kernel_ms[k];
  return ARTIS_OK;
}

}  // extern "C"
