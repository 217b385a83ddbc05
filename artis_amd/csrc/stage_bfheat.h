// stage_bfheat.h -- artis_amd_bfheating_*: the bound-free heating coefficients of the thin (fitted) cells on the device, and
// artis_amd_thermal_solve_bfheated, the thermal solve (stage_thermal.h) reading them where they lie (rules and bodies: bf_heating.h).
// Kernels on the caller's stream: k_bfh_ground (one lane per (cell, ground continuum): the renormalisation factors, from the RESIDENT
// T_R and W) and k_bfh_levels (one lane per (fitted cell, level that has targets), with the fit's T_R and W; the levels of one cell sit on
// neighbouring lanes, so a wave reads one cell's T_R, W and renormalisation row). One lane per level, not one wave per integral: the
// adaptive walk ends after its first node (bf_heating.h), so a lane runs 61 independent evaluations with no cross-lane step and the
// reference's summation order comes for free. k_bfh_levels is launched in batches of BFH_BATCH_CELLS cells: no launch's length depends on
// the whole grid. The block is cleared on the stream before the kernels (+0 for unfitted cells and levels without targets); after
// that every element has one writer. Flags are integer ORs; the totals (nodes evaluated, integrals that subdivided, that reached depth
// 15, non-finite coefficients) are integers, summed per wave behind one ballot each and added by the wave's first lane.
#pragma once

namespace {

constexpr int64_t BFH_BATCH_CELLS = 4096;

#if ARTIS_TB_SUPPORTED

struct BfhArgs {
  artis::DevModel M;
  artis_bfh::Arrays A;
  const int32_t *cells;  // k_bfh_levels: the fitted cells
  int64_t cell0;         // ... the launch's first entry of that list
  int32_t ncells;        // ... and how many it takes
  unsigned long long *totals;
};

// the wave's sums of the lanes' totals; every lane of the wave arrives here
__device__ inline void bfh_wave_totals(const artis_bfh::Totals &t, unsigned long long *totals) {
  for (int k = 0; k < artis_bfh::NTOTALS; k++) {
    long long v = t.v[k];
    if (__ballot(v != 0) == 0) continue;  // (wave-uniform)
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&totals[k], (unsigned long long)v);
  }
}

__global__ void __launch_bounds__(BLOCK) k_bfh_ground(BfhArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  artis_bfh::Totals tot{};
  if (i < a.A.ncell * a.A.nbfg) {
    const int64_t c = i / a.A.nbfg;
    const int32_t flag = artis_bfh::ground_cell_entry(a.M, a.A, c, (int)(i - c * a.A.nbfg), &tot);
    if (flag) atomicOr(&a.A.flags[c], flag);
  }
  bfh_wave_totals(tot, a.totals);
}

__global__ void __launch_bounds__(BLOCK) k_bfh_levels(BfhArgs a) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  artis_bfh::Totals tot{};
  if (i < (int64_t)a.ncells * a.A.nlevels_listed) {
    const int64_t j = i / a.A.nlevels_listed;
    const int64_t c = a.cells[a.cell0 + j];
    const int32_t flag = artis_bfh::level_cell_entry(a.M, a.A, c, (int)(i - j * a.A.nlevels_listed), &tot);
    if (flag) atomicOr(&a.A.flags[c], flag);
  }
  bfh_wave_totals(tot, a.totals);
}

#endif  // ARTIS_TB_SUPPORTED

__global__ void __launch_bounds__(BLOCK) k_gk61_debug(const int32_t ncases, const artis_gk61_case *cases, artis_gk61_result *out) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= ncases) return;
  const artis_gk61_case cs = cases[i];
  int64_t evals = 0;
  const artis_bfh::Gk61TestFn f{cs.which, cs.p, &evals};
  artis_bfh::Gk61Stats st;
  double error = 0.;
  const double r = artis_bfh::gk61_integrate(f, cs.a, cs.b, cs.tol, &error, &st);
  out[i].result = r;
  out[i].error = error;
  out[i].evals = evals;
  out[i].nodes = st.nodes;
  out[i].maxdepth = st.maxdepth;
}

// everything of artis_amd_bfheating_*: one block, made at the first call
struct BfhState {
  StageBlock block;
  int64_t ncell = 0, nlevels = 0, nbfg = 0, nlisted = 0, nground = 0, ntargets = 0;
  double *d_coeffs = nullptr, *d_renorm = nullptr;
  float *d_TR = nullptr, *d_W = nullptr;  // the caller's T_R and W of a call that gave them
  int32_t *d_flags = nullptr, *d_cells = nullptr, *d_levels = nullptr;
  unsigned long long *d_totals = nullptr;
  bool valid = false;
  uint64_t fit_serial = 0;        // the fit the last update was made on
  uint64_t cellstate_serial = 0;  // ... and the resident cell state it read
  int64_t nfitted = 0;
  unsigned long long totals[artis_bfh::NTOTALS] = {};
  double kernel_ms[ARTIS_BFHEAT_NTIMES] = {};
};

void bfh_free(BfhState *st) { delete st; }

#if ARTIS_TB_SUPPORTED

// after tb_alpha_sp (the ground-continuum indices exist)
int bfh_init(artis_amd_engine *e) {
  if (e->bfh) return ARTIS_OK;
  const DevModel &h = e->Mh;
  BfhState *st = new BfhState();
  const int64_t n = st->ncell = h.npts_nonempty, nl = st->nlevels = h.nlevels, g = st->nbfg = h.nbfcontinua_ground;
  std::vector<int32_t> nt((size_t)(nl > 0 ? nl : 1)), gci((size_t)(h.nions > 0 ? h.nions : 1)), levels;
  hipError_t err = hipSuccess;
  if (nl > 0) err = hipMemcpy(nt.data(), e->M.level_nphixstargets, sizeof(int32_t) * (size_t)nl, hipMemcpyDeviceToHost);
  if (err == hipSuccess && h.nions > 0) err = hipMemcpy(gci.data(), e->ib->d_gci, sizeof(int32_t) * (size_t)h.nions, hipMemcpyDeviceToHost);
  if (err != hipSuccess) {
    delete st;
    return stage_error(ARTIS_ERR_HIP, std::string("bfheating: the levels' targets: ") + hipGetErrorString(err));
  }
  for (int64_t ul = 0; ul < nl; ul++)
    if (nt[(size_t)ul] > 0) {
      levels.push_back((int32_t)ul);
      st->ntargets += nt[(size_t)ul];
    }
  for (int ui = 0; ui < h.nions; ui++) st->nground += gci[(size_t)ui] >= 0;
  st->nlisted = (int64_t)levels.size();
  const int rc = st->block.make({piece(&st->d_coeffs, n * nl), piece(&st->d_renorm, n * g), piece(&st->d_TR, n), piece(&st->d_W, n), piece(&st->d_flags, n),
                                 piece(&st->d_cells, n), piece(&st->d_levels, st->nlisted), piece(&st->d_totals, artis_bfh::NTOTALS)},
                                "bfheating", "the result block");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  err = stage_copy(st->d_levels, levels.data(), st->nlisted, hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    delete st;
    return stage_error(ARTIS_ERR_HIP, std::string("bfheating: the list of levels: ") + hipGetErrorString(err));
  }
  e->bfh = st;
  return ARTIS_OK;
}

#endif  // ARTIS_TB_SUPPORTED

}  // namespace

extern "C" {

int artis_amd_bfheating_update(artis_amd_engine *e, const artis_bfheating_params *p, void *hip_stream) {
  if (!e || !p) return stage_error(ARTIS_ERR_ARG, "bfheating_update: null engine or parameters");
#if !ARTIS_TB_SUPPORTED
  return tb_unsupported("bfheating_update");
#else
  STAGE_STRUCT_SIZE(p, artis_bfheating_params, "bfheating_update");
  if (!e->have_cells) return stage_error(ARTIS_ERR_ARG, "bfheating_update: no cell state (artis_amd_set_cellstate)");
  if (!e->rf || !e->rf->valid || !e->fit_since_step)
    return stage_error(ARTIS_ERR_ARG, "bfheating_update: needs an artis_amd_radfield_fit since the last propagation call");
  if ((p->TR != nullptr) != (p->W != nullptr)) return stage_error(ARTIS_ERR_ARG, "bfheating_update: TR and W come together or not at all");
  if (!ARTIS_OPT_USE_ION_BFHEATING_ESTIMATORS && !e->C.elem_massfracs)
    return stage_error(ARTIS_ERR_ARG, "bfheating_update: this build has no USE_ION_BFHEATING_ESTIMATORS: the cell state needs elem_massfracs");
  hipStream_t s = (hipStream_t)hip_stream;
  HIP_TRY(hipSetDevice(e->device));
  int rc = tb_alpha_sp(e, s);
  if (rc != ARTIS_OK) return rc;
  if ((rc = bfh_init(e)) != ARTIS_OK) return rc;
  BfhState *st = e->bfh;
  st->valid = false;
  const int64_t n = st->ncell, nl = st->nlevels, g = st->nbfg;
  if (p->TR) {
    HIP_TRY(stage_copy(st->d_TR, p->TR, n, hipMemcpyHostToDevice, &s));
    HIP_TRY(stage_copy(st->d_W, p->W, n, hipMemcpyHostToDevice, &s));
  }
  // the fitted cells, in cell order
  std::vector<int32_t> fit_flags((size_t)(n > 0 ? n : 1)), cells;
  HIP_TRY(stage_copy(fit_flags.data(), e->rf->d_flags, n, hipMemcpyDeviceToHost, &s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int64_t c = 0; c < n; c++)
    if (fit_flags[(size_t)c] & ARTIS_RADFIELD_FITTED) cells.push_back((int32_t)c);
  st->nfitted = (int64_t)cells.size();
  HIP_TRY(stage_copy(st->d_cells, cells.data(), st->nfitted, hipMemcpyHostToDevice, &s));
  if (n * nl > 0) HIP_TRY(hipMemsetAsync(st->d_coeffs, 0, sizeof(double) * (size_t)(n * nl), s));
  if (n > 0) HIP_TRY(hipMemsetAsync(st->d_flags, 0, sizeof(int32_t) * (size_t)n, s));
  HIP_TRY(hipMemsetAsync(st->d_totals, 0, sizeof(unsigned long long) * artis_bfh::NTOTALS, s));
  BfhArgs a{};
  a.M = e->M;
  artis_bfh::Arrays &A = a.A;
  A.ncell = n;
  A.nbfg = (int32_t)g;
  A.res_TR = e->C.TR;
  A.res_W = e->C.W;
  A.lev_TR = p->TR ? st->d_TR : e->rf->d_TR;
  A.lev_W = p->TR ? st->d_W : e->rf->d_W;
  A.fit_flags = e->rf->d_flags;
  A.bfh_raw = e->E.bfheatingestimator;
  A.bfh_stride = 2;
  A.assocvol = e->rf->d_assocvol;
  A.prev_mid = e->rf->prev_mid;
  A.tmin = e->model_copy.tmin;
  A.deltat = e->rf->deltat;
  A.nprocs = e->rf->nprocs;
  A.gci = e->ib->d_gci;
  A.massfrac = ARTIS_OPT_USE_ION_BFHEATING_ESTIMATORS ? nullptr : e->C.elem_massfracs;
  A.levels = st->d_levels;
  A.nlevels_listed = (int32_t)st->nlisted;
  A.renorm = st->d_renorm;
  A.coeffs = st->d_coeffs;
  A.flags = st->d_flags;
  a.cells = st->d_cells;
  a.totals = st->d_totals;
  auto launched = [&](const char *kernel, hipError_t err) -> int {
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("bfheating_update: ") + kernel + ": " + hipGetErrorString(err));
    return ARTIS_OK;
  };
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  if (n > 0 && g > 0) {
    hipLaunchKernelGGL(k_bfh_ground, dim3(nblocks(n * g)), dim3(BLOCK), 0, s, a);
    if ((rc = launched("k_bfh_ground", hipGetLastError())) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[1], s));
  for (int64_t c0 = 0; c0 < st->nfitted && st->nlisted > 0; c0 += BFH_BATCH_CELLS) {
    a.cell0 = c0;
    a.ncells = (int32_t)std::min(BFH_BATCH_CELLS, st->nfitted - c0);
    hipLaunchKernelGGL(k_bfh_levels, dim3(nblocks((int64_t)a.ncells * st->nlisted)), dim3(BLOCK), 0, s, a);
    if ((rc = launched("k_bfh_levels", hipGetLastError())) != ARTIS_OK) return rc;
  }
  HIP_TRY(hipEventRecord(st->block.ev[2], s));
  HIP_TRY(hipMemcpyAsync(st->totals, st->d_totals, sizeof(st->totals), hipMemcpyDeviceToHost, s));
  {
    const hipError_t err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("bfheating_update: a kernel of the call: ") + hipGetErrorString(err));
  }
  for (int k = 0; k < ARTIS_BFHEAT_NTIMES; k++) HIP_TRY(st->block.elapsed_ms(k, &st->kernel_ms[k]));
  if (st->totals[3] > 0)
    return stage_error(ARTIS_ERR_NOTCONVERGED, "bfheating_update: " + std::to_string(st->totals[3]) + " coefficients are not finite: the block is refused");
  st->fit_serial = e->rf->serial;
  st->cellstate_serial = e->cellstate_serial;
  st->valid = true;
  return ARTIS_OK;
#endif
}

int artis_amd_bfheating_download(artis_amd_engine *e, artis_bfheating_result *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "bfheating_download: null argument");
#if !ARTIS_TB_SUPPORTED
  return tb_unsupported("bfheating_download");
#else
  STAGE_STRUCT_SIZE(out, artis_bfheating_result, "bfheating_download");
  if (!e->bfh || !e->bfh->valid) return stage_error(ARTIS_ERR_ARG, "bfheating_download: nothing computed (artis_amd_bfheating_update)");
  BfhState *st = e->bfh;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell;
  HIP_TRY(stage_copy(out->coeffs, st->d_coeffs, n * st->nlevels, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->renorm, st->d_renorm, n * st->nbfg, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->flags, st->d_flags, n, hipMemcpyDeviceToHost));
  for (int k = 0; k < ARTIS_BFHEAT_NTOTALS; k++) out->totals[k] = (int64_t)st->totals[k];
  out->nfitted = st->nfitted;
  out->nintegrals = st->nfitted * (st->ntargets + st->nground);
  out->npts_nonempty = (int32_t)n;
  out->nlevels = (int32_t)st->nlevels;
  out->nbfcontinua_ground = (int32_t)st->nbfg;
  out->nlevels_with_targets = (int32_t)st->nlisted;
  for (int k = 0; k < ARTIS_BFHEAT_NTIMES; k++) out->kernel_ms[k] = st->kernel_ms[k];
  return ARTIS_OK;
#endif
}

int artis_amd_thermal_solve_bfheated(artis_amd_engine *e, const artis_thermal_params *p, void *hip_stream) {
  if (!e || !p) return stage_error(ARTIS_ERR_ARG, "thermal_solve_bfheated: null engine or parameters");
#if !ARTIS_TB_SUPPORTED
  return tb_unsupported("thermal_solve_bfheated");
#else
  STAGE_STRUCT_SIZE(p, artis_thermal_params, "thermal_solve_bfheated");
  if (p->bfheatingcoeffs) return stage_error(ARTIS_ERR_ARG, "thermal_solve_bfheated: bfheatingcoeffs must be NULL (the coefficients are the last artis_amd_bfheating_update's)");
  if (!e->bfh || !e->bfh->valid || !e->rf || !e->rf->valid || e->bfh->fit_serial != e->rf->serial || e->bfh->cellstate_serial != e->cellstate_serial)
    return stage_error(ARTIS_ERR_ARG, "thermal_solve_bfheated: no artis_amd_bfheating_update on the last artis_amd_radfield_fit and the resident cell state");
  return tb_solve(e, p, hip_stream, e->bfh->d_coeffs);
#endif
}

int artis_amd_debug_gk61(int32_t ncases, const artis_gk61_case *cases, artis_gk61_result *out) {
  if (ncases < 0 || (ncases > 0 && (!cases || !out))) return stage_error(ARTIS_ERR_ARG, "debug_gk61: null argument");
  if (ncases == 0) return ARTIS_OK;
  artis_gk61_case *d_cases = nullptr;
  artis_gk61_result *d_out = nullptr;
  hipError_t err = hipMalloc(&d_cases, sizeof(artis_gk61_case) * (size_t)ncases);
  if (err == hipSuccess) err = hipMalloc(&d_out, sizeof(artis_gk61_result) * (size_t)ncases);
  if (err == hipSuccess) err = hipMemcpy(d_cases, cases, sizeof(artis_gk61_case) * (size_t)ncases, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_gk61_debug, dim3(nblocks(ncases)), dim3(BLOCK), 0, 0, ncases, d_cases, d_out);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out, d_out, sizeof(artis_gk61_result) * (size_t)ncases, hipMemcpyDeviceToHost);
  if (d_cases) (void)hipFree(d_cases);
  if (d_out) (void)hipFree(d_out);
  if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("debug_gk61: ") + hipGetErrorString(err));
  return ARTIS_OK;
}

}  // extern "C"
