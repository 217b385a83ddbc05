// stage_photoion.h -- artis_amd_set_cellstate_photoion / artis_amd_photoion_download: the photoionisation coefficients of builds
// without USE_LUT_PHOTOION on the device, between the two halves of artis_amd_set_cellstate (rules and bodies: photoion.h).
// One kernel on the caller's stream, k_photoion: one lane per (cell, continuum of the allcont_* arrays); a workgroup (one wave) serves one
// cell at a time -- blockIdx.y is the cell of the launch, blockIdx.x the run of PI_BLOCK continua -- so its lanes share the cell's T_e,
// n_e, Tepow and radiation field, and it stages the cell's RADFIELDBINCOUNT (W, T_R) pairs in LDS (2 KB at 256 bins), where the
// integrand's 61 evaluations per lane read the bin radbin_select gives. One wave per workgroup: with 159 continua a cell fills 2.5 waves,
// and a workgroup of 256 lanes would leave 38 % of them without a continuum; the staging is 4 reads per lane against 61 evaluations of some hundred
// operations each. Launched in batches of PI_BATCH_CELLS cells: no launch's length depends on the grid. The block is cleared on the
// stream first (+0 and source 0 for entries no continuum writes); after that every element has one writer. Flags are integer ORs; the
// totals are integers, summed per wave behind one ballot each and added by the wave's first lane.
#pragma once

namespace {

constexpr int PI_BLOCK = 64;
constexpr int64_t PI_BATCH_CELLS = 4096;  // (gridDim.y: at most 65535)

struct PiArgs {
  artis::DevModel M;
  artis_pi::Arrays A;
  int64_t cell0;  // the launch's first cell
  unsigned long long *totals;
};

__global__ void __launch_bounds__(PI_BLOCK) k_photoion(PiArgs a) {
  __shared__ artis_pi::BinWT bins[artis_pi::NBINS];
  const int64_t c = a.cell0 + blockIdx.y;  // < ncell: the launch's gridDim.y is the batch's number of cells
  if (ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON && a.A.binned) {
    for (int b = threadIdx.x; b < artis_pi::NBINS; b += PI_BLOCK) artis_pi::stage_bin(a.A, c, b, bins);
    __syncthreads();
  }
  const int i = blockIdx.x * PI_BLOCK + threadIdx.x;
  artis_pi::Totals tot{};
  if (i < a.A.ncont) {
    const artis_pi::CellIn cell = artis_pi::cell_in(a.M, a.A, c);
    const artis_pi::CellRadfield<artis_pi::TbMath> J = artis_pi::cell_radfield<artis_pi::TbMath>(a.A, c, bins);
    const int32_t flag = artis_pi::cont_cell_entry<artis_pi::TbMath>(a.M, a.A, c, i, cell, J, &tot);
    if (flag) atomicOr(&a.A.flags[c], flag);
  }
  // the wave's sums of the lanes' totals; every lane of the wave arrives here
  for (int k = 0; k < artis_pi::NTOTALS; k++) {
    long long v = tot.v[k];
    if (__ballot(v != 0) == 0) continue;  // (wave-uniform)
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&a.totals[k], (unsigned long long)v);
  }
}

// everything of the call besides the coefficients (those live among the cell allocations): one block, made at the first call
struct PiState {
  StageBlock block;
  int64_t ncell = 0, nentries = 0, ncont = 0, nbf = 0;
  uint8_t *d_source = nullptr;
  int32_t *d_flags = nullptr;
  double *d_Tepow = nullptr;
  float *d_bf = nullptr;  // the caller's bfrate_normed of a call that gave one
  unsigned long long *d_totals = nullptr;
  bool valid = false;
  unsigned long long totals[artis_pi::NTOTALS] = {};
  double kernel_ms = 0.;
};

void pi_free(PiState *st) { delete st; }

int pi_init(artis_amd_engine *e) {
  if (e->pi) return ARTIS_OK;
  const DevModel &h = e->Mh;
  PiState *st = new PiState();
  const int64_t n = st->ncell = h.npts_nonempty;
  st->nentries = h.nphixstargets_total;
  st->ncont = h.nbfcontinua;
  st->nbf = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? h.nbfestim : 0;
  const int rc = st->block.make({piece(&st->d_source, n * st->nentries), piece(&st->d_flags, n), piece(&st->d_Tepow, n), piece(&st->d_bf, n * st->nbf),
                                 piece(&st->d_totals, artis_pi::NTOTALS)},
                                "set_cellstate_photoion", "the result block");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  e->pi = st;
  return ARTIS_OK;
}

}  // namespace

extern "C" {

int artis_amd_set_cellstate_photoion(artis_amd_engine *e, const artis_cellstate *cells, const artis_timestep *ts, const artis_photoion_params *p,
                                     void *hip_stream) {
  if (!e || !cells || !ts || !p) return stage_error(ARTIS_ERR_ARG, "set_cellstate_photoion: null argument");
  if (p->struct_size != sizeof(artis_photoion_params))
    return stage_error(ARTIS_ERR_ARG, "set_cellstate_photoion: artis_photoion_params.struct_size does not match");
  if (p->use_bf_estimators != 0 && p->use_bf_estimators != 1) return stage_error(ARTIS_ERR_ARG, "set_cellstate_photoion: use_bf_estimators must be 0 or 1");
  if (p->use_bf_estimators && !ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON)
    return stage_error(ARTIS_ERR_ARG, "set_cellstate_photoion: use_bf_estimators in a build without DETAILED_BF_ESTIMATORS_ON");
  if (ARTIS_OPT_USE_LUT_PHOTOION)
    return stage_error(ARTIS_ERR_UNSUPPORTED, "set_cellstate_photoion: this build has USE_LUT_PHOTOION: the coefficients come from the model's table (artis_amd_set_cellstate)");
  if (cells->corrphotoioncoeff)
    return stage_error(ARTIS_ERR_ARG, "set_cellstate_photoion: artis_cellstate.corrphotoioncoeff must be NULL (the engine computes it; artis_amd_set_cellstate takes a host array)");
  if (p->cells_per_launch < 0) return stage_error(ARTIS_ERR_ARG, "set_cellstate_photoion: cells_per_launch must not be negative");
  if (!cells->levelpops) return stage_error(ARTIS_ERR_ARG, "set_cellstate_photoion: artis_cellstate.levelpops is required (the departure ratios)");
  const DevModel &h = e->Mh;
  const int64_t nbf = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? h.nbfestim : 0;
  const bool from_fit = p->use_bf_estimators && !p->bfrate_normed;
  if (from_fit && (!e->rf || !e->rf->valid || !e->rf->d_bf || e->rf->nbf != nbf))
    return stage_error(ARTIS_ERR_ARG, "set_cellstate_photoion: use_bf_estimators with bfrate_normed NULL needs a valid artis_amd_radfield_fit (its bfrate_normed)");
  hipStream_t s = (hipStream_t)hip_stream;
  HIP_TRY(hipSetDevice(e->device));
  int rc = pi_init(e);
  if (rc != ARTIS_OK) return rc;
  PiState *st = e->pi;
  st->valid = false;
  if ((rc = cellstate_upload(e, cells, ts, true)) != ARTIS_OK) return rc;  // (the multibin build's bins are checked there)
  const int64_t n = st->ncell, ne = st->nentries;
  // the coefficients: among the cell allocations, as the host's array would be
  double *d_coeff = nullptr;
  HIP_TRY(hipMalloc((void **)&d_coeff, sizeof(double) * (size_t)(n * ne > 0 ? n * ne : 1)));
  e->cell_allocs.push_back(d_coeff);
  e->pi_coeff = d_coeff;
  {
    std::vector<double> Tepow((size_t)(n > 0 ? n : 1));
    artis_pi::make_tepow(cells->Te, n, Tepow.data());
    HIP_TRY(stage_copy(st->d_Tepow, Tepow.data(), n, hipMemcpyHostToDevice));
  }
  if (p->use_bf_estimators && p->bfrate_normed) HIP_TRY(stage_copy(st->d_bf, p->bfrate_normed, n * nbf, hipMemcpyHostToDevice));
  if (n * ne > 0) {
    HIP_TRY(hipMemsetAsync(d_coeff, 0, sizeof(double) * (size_t)(n * ne), s));
    HIP_TRY(hipMemsetAsync(st->d_source, 0, (size_t)(n * ne), s));
  }
  if (n > 0) HIP_TRY(hipMemsetAsync(st->d_flags, 0, sizeof(int32_t) * (size_t)n, s));
  HIP_TRY(hipMemsetAsync(st->d_totals, 0, sizeof(unsigned long long) * artis_pi::NTOTALS, s));
  PiArgs a{};
  a.M = e->M;
  artis_pi::Arrays &A = a.A;
  A.ncell = n;
  A.ncont = (int32_t)st->ncont;
  A.nentries = (int32_t)ne;
  A.nbfestim = (int32_t)nbf;
  A.use_bf_estimators = p->use_bf_estimators;
  A.binned = ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON && ts->nts >= ARTIS_OPT_FIRST_NLTE_RADFIELD_TIMESTEP;
  A.Te = e->C.Te;
  A.nne = e->C.nne;
  A.clumpfactor = e->C.clumpfactor;
  A.TR = e->C.TR;
  A.W = e->C.W;
  A.Tepow = st->d_Tepow;
  A.levelpops = e->C.levelpops;
  A.bin_W = e->C.radfieldbin_W;
  A.bin_T_R = e->C.radfieldbin_T_R;
  A.bfrate_normed = !p->use_bf_estimators ? nullptr : (from_fit ? e->rf->d_bf : st->d_bf);
  A.coeff = d_coeff;
  A.source = st->d_source;
  A.flags = st->d_flags;
  a.totals = st->d_totals;
  const int64_t per_launch = p->cells_per_launch > 0 ? std::min<int64_t>(p->cells_per_launch, PI_BATCH_CELLS) : PI_BATCH_CELLS;
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  for (int64_t c0 = 0; c0 < n && st->ncont > 0; c0 += per_launch) {
    a.cell0 = c0;
    const int64_t ncells = std::min(per_launch, n - c0);
    hipLaunchKernelGGL(k_photoion, dim3((unsigned)((st->ncont + PI_BLOCK - 1) / PI_BLOCK), (unsigned)ncells), dim3(PI_BLOCK), 0, s, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("set_cellstate_photoion: k_photoion: ") + hipGetErrorString(err));
  }
  HIP_TRY(hipEventRecord(st->block.ev[1], s));
  HIP_TRY(hipMemcpyAsync(st->totals, st->d_totals, sizeof(st->totals), hipMemcpyDeviceToHost, s));
  {
    const hipError_t err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("set_cellstate_photoion: k_photoion: ") + hipGetErrorString(err));
  }
  HIP_TRY(st->block.elapsed_ms(0, &st->kernel_ms));
  st->valid = true;
  if (st->totals[4] > 0)
    return stage_error(ARTIS_ERR_NOTCONVERGED, "set_cellstate_photoion: " + std::to_string(st->totals[4]) + " coefficients are not finite: no cell state is set");
  e->C.corrphotoioncoeff = d_coeff;
  return cellstate_finish(e);
}

int artis_amd_photoion_download(artis_amd_engine *e, artis_photoion_result *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "photoion_download: null argument");
  STAGE_STRUCT_SIZE(out, artis_photoion_result, "photoion_download");
  if (!e->pi || !e->pi->valid || !e->pi_coeff)
    return stage_error(ARTIS_ERR_ARG, "photoion_download: nothing computed for the cell state that was set last (artis_amd_set_cellstate_photoion)");
  PiState *st = e->pi;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell, ne = st->nentries;
  HIP_TRY(stage_copy(out->coeff, e->pi_coeff, n * ne, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->source, st->d_source, n * ne, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->flags, st->d_flags, n, hipMemcpyDeviceToHost));
  for (int k = 0; k < artis_pi::NTOTALS; k++) out->totals[k] = (int64_t)st->totals[k];
  out->npts_nonempty = (int32_t)n;
  out->nphixstargets_total = (int32_t)ne;
  out->nbfcontinua = (int32_t)st->ncont;
  out->nbfestim = (int32_t)st->nbf;
  out->kernel_ms = st->kernel_ms;
  return ARTIS_OK;
}

}  // extern "C"
