// stage_radfield.h -- artis_amd_radfield_*: the radiation-field fit (rules and per-element bodies: radfield_fit.h).
// Two kernels on the caller's stream. k_rf_cell: one wave per cell; lane 0 normalises J (and nuJ) and fits T_J, T_R, W
// (artis_rf::fit_cell_store), the wave's lanes normalise the cell's bound-free and line estimators and carry the bins of a cell
// that is not fitted over from the cell state. k_rf_bins: one lane per (cell, bin), a cell's bins on neighbouring lanes so that
// a wave's residuals have similar x; the estimators are read in place ([cell][bin]{J, nuJ}). Nothing is added with float
// atomics: every output element has one writer. The bin counts are integer atomics (per cell, only for a bin that has the
// bit) and one ballot per wave and count for the totals.
#pragma once

namespace {

struct RfArgs {
  int64_t ncell;
  // inputs: the estimator block (J, nuJ with stride 8), the cell state, the caller's volumes
  const double *J_raw, *nuJ_raw, *bin_est, *bfrate_raw, *Jb_raw, *Jb_count;
  const double *assocvol;
  const int32_t *thick;
  const float *TJ, *TR, *Te, *W, *prev_bin_T_R, *prev_bin_W;
  double prev_mid, tmin, deltat;
  int32_t nprocs, lte, nbf, nline;
  // outputs
  artis_rf::CellArrays cell;
  float *bin_T_R, *bin_W, *bf;
  double *Jb, *Jbcount;
  unsigned long long *totals;
};

__global__ void __launch_bounds__(BLOCK) k_rf_cell(RfArgs a) {
  using namespace artis_rf;
  const int64_t c = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) / 64;
  const int lane = (int)(threadIdx.x & 63);
  if (c >= a.ncell) return;  // whole waves
  const int32_t thick = a.thick[c];
  if (lane == 0)
    fit_cell_store(c, CellIn{a.J_raw[c * 8], a.nuJ_raw[c * 8], a.assocvol[c], a.prev_mid, a.tmin, a.deltat, a.nprocs, a.lte, thick,
                             a.TJ[c], a.TR[c], a.Te[c], a.W[c]},
                   a.cell);
  double estimator_normfactor, over4pi;
  cell_normfactors(a.assocvol[c], a.prev_mid, a.tmin, a.deltat, a.nprocs, &estimator_normfactor, &over4pi);
  if (a.bin_T_R && cell_bins_carried_over(a.lte, thick))
    for (int b = lane; b < NBINS; b += 64) carry_bin(c * NBINS + b, a.prev_bin_T_R, a.prev_bin_W, a.bin_T_R, a.bin_W);
  if (a.bf && cell_bf_rewritten(a.lte, thick))
    for (int i = lane; i < a.nbf; i += 64) bf_entry(c * a.nbf + i, a.bfrate_raw, estimator_normfactor, a.bf);
  if (a.Jb)
    for (int i = lane; i < a.nline; i += 64) line_entry(c * a.nline + i, a.Jb_raw, a.Jb_count, over4pi, a.Jb, a.Jbcount);
}

__global__ void __launch_bounds__(BLOCK) k_rf_bins(RfArgs a) {
  using namespace artis_rf;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int bits = 0;
  if (i < a.ncell * NBINS) {
    bits = fit_bin_store(i, &a.bin_est[2 * i], &a.bin_est[2 * i + 1], a.cell.flags, a.cell.J_normfactor, a.Te, a.bin_T_R, a.bin_W);
    for (int k = 0; k < ARTIS_RADFIELD_NCOUNTS; k++)
      if (bits & (1 << k)) atomicAdd(&a.cell.counts[(i / NBINS) * ARTIS_RADFIELD_NCOUNTS + k], 1);
  }
  for (int k = 0; k < ARTIS_RADFIELD_NCOUNTS; k++) {  // the bit k of a bin is count k (artis_rf::BIN_*)
    const unsigned long long m = __ballot((bits >> k) & 1);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.totals[k], (unsigned long long)__popcll(m));
  }
}

// the result block of artis_amd_radfield_*: made at the first call, zeroed then (the bound-free block keeps its values from
// call to call for the THICK cells, as the reference's prev_bfrate_normed does)
struct RfState {
  StageBlock block;
  int64_t ncell = 0, nbins = 0, nbf = 0, nline = 0;
  double *d_J = nullptr, *d_nuJ = nullptr, *d_normfactor = nullptr, *d_assocvol = nullptr, *d_Jb = nullptr, *d_Jbcount = nullptr;
  float *d_TJ = nullptr, *d_TR = nullptr, *d_Te = nullptr, *d_W = nullptr, *d_bin_T_R = nullptr, *d_bin_W = nullptr, *d_bf = nullptr;
  int32_t *d_flags = nullptr, *d_counts = nullptr;
  unsigned long long *d_totals = nullptr;
  bool valid = false;
  uint64_t serial = 0;  // counts the fits (artis_amd_grid_update_thermal: was the thermal solve made on the last one)
  double prev_mid = 0., deltat = 0.;  // the normalisation of the last fit (artis_amd_grid_update reads it)
  int32_t nprocs = 1, lte = 0;
  unsigned long long totals[ARTIS_RADFIELD_NCOUNTS] = {};
  double kernel_ms[2] = {};
};

void rf_free(RfState *st) { delete st; }

int rf_init(artis_amd_engine *e) {
  if (e->rf) return ARTIS_OK;
  RfState *st = new RfState();
  const int64_t n = st->ncell = e->Mh.npts_nonempty;
  st->nbins = ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON ? ARTIS_OPT_RADFIELDBINCOUNT : 0;
  st->nbf = e->E.bfrate_raw ? e->Mh.nbfestim : 0;
  st->nline = e->E.Jb_lu_raw ? e->Mh.detailed_linecount : 0;
  const int rc = st->block.make(
      {piece(&st->d_J, n), piece(&st->d_nuJ, n), piece(&st->d_normfactor, n), piece(&st->d_assocvol, n), piece(&st->d_TJ, n),
       piece(&st->d_TR, n), piece(&st->d_Te, n), piece(&st->d_W, n), piece(&st->d_flags, n),
       piece(&st->d_counts, n * ARTIS_RADFIELD_NCOUNTS), piece(&st->d_totals, ARTIS_RADFIELD_NCOUNTS),
       piece(&st->d_bin_T_R, n * st->nbins), piece(&st->d_bin_W, n * st->nbins), piece(&st->d_bf, n * st->nbf),
       piece(&st->d_Jb, n * st->nline), piece(&st->d_Jbcount, n * st->nline)},
      "radfield", "the result block");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  e->rf = st;
  return ARTIS_OK;
}

}  // namespace

extern "C" {

int artis_amd_radfield_fit(artis_amd_engine *e, const artis_radfield_config *cfg, void *hip_stream) {
  if (!e || !cfg) return stage_error(ARTIS_ERR_ARG, "radfield: null engine or config");
  STAGE_STRUCT_SIZE(cfg, artis_radfield_config, "radfield");
  if (!e->have_cells) return stage_error(ARTIS_ERR_ARG, "radfield: no cell state (artis_amd_set_cellstate)");
  if (!(cfg->deltat > 0) || !std::isfinite(cfg->deltat)) return stage_error(ARTIS_ERR_ARG, "radfield: deltat must be positive and finite");
  if (!(cfg->prev_mid > 0) || !std::isfinite(cfg->prev_mid)) return stage_error(ARTIS_ERR_ARG, "radfield: prev_mid must be positive and finite");
  if (cfg->nprocs < 1) return stage_error(ARTIS_ERR_ARG, "radfield: nprocs < 1");
  if (!cfg->assocvolume_tmin) return stage_error(ARTIS_ERR_ARG, "radfield: null assocvolume_tmin");
  const int64_t ncell = e->Mh.npts_nonempty;
  for (int64_t c = 0; c < ncell; c++)
    if (!(cfg->assocvolume_tmin[c] > 0) || !std::isfinite(cfg->assocvolume_tmin[c]))
      return stage_error(ARTIS_ERR_ARG, "radfield: assocvolume_tmin must be positive and finite in every cell");
  if (e->E.bfrate_raw && e->bfrate_kept_dirty)
    return stage_error(ARTIS_ERR_ARG, "radfield: the last propagation call ended in an error, the bound-free estimators are incomplete");
  HIP_TRY(hipSetDevice(e->device));
  int rc = rf_init(e);
  if (rc != ARTIS_OK) return rc;
  RfState *st = e->rf;
  st->valid = false;
  hipStream_t s = (hipStream_t)hip_stream;
  HIP_TRY(stage_copy(st->d_assocvol, cfg->assocvolume_tmin, ncell, hipMemcpyHostToDevice, &s));
  HIP_TRY(stage_copy(st->d_bf, cfg->bfrate_normed_seed, ncell * st->nbf, hipMemcpyHostToDevice, &s));
  HIP_TRY(hipMemsetAsync(st->d_totals, 0, sizeof(unsigned long long) * ARTIS_RADFIELD_NCOUNTS, s));
  RfArgs a{};
  a.ncell = ncell;
  a.J_raw = e->E.J;
  a.nuJ_raw = e->E.nuJ;
  a.bin_est = e->E.radfieldbin_J;
  a.bfrate_raw = e->E.bfrate_raw;
  a.Jb_raw = e->E.Jb_lu_raw;
  a.Jb_count = e->E.Jb_lu_contribcount;
  a.assocvol = st->d_assocvol;
  a.thick = e->C.thick;
  a.TJ = e->C.TJ;
  a.TR = e->C.TR;
  a.Te = e->C.Te;
  a.W = e->C.W;
  a.prev_bin_T_R = e->C.radfieldbin_T_R;
  a.prev_bin_W = e->C.radfieldbin_W;
  a.prev_mid = cfg->prev_mid;
  a.tmin = e->model_copy.tmin;
  a.deltat = cfg->deltat;
  a.nprocs = cfg->nprocs;
  a.lte = cfg->lte_iteration != 0;
  a.nbf = (int32_t)st->nbf;
  a.nline = (int32_t)st->nline;
  a.cell = {st->d_J, st->d_nuJ, st->d_normfactor, st->d_TJ, st->d_TR, st->d_Te, st->d_W, st->d_flags, st->d_counts};
  a.bin_T_R = st->d_bin_T_R;
  a.bin_W = st->d_bin_W;
  a.bf = st->d_bf;
  a.Jb = st->d_Jb;
  a.Jbcount = st->d_Jbcount;
  a.totals = st->d_totals;
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  if (ncell > 0) {
    hipLaunchKernelGGL(k_rf_cell, dim3(nblocks(ncell * 64)), dim3(BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(st->block.ev[1], s));
  if (ncell > 0 && st->nbins > 0) {
    hipLaunchKernelGGL(k_rf_bins, dim3(nblocks(ncell * st->nbins)), dim3(BLOCK), 0, s, a);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(st->block.ev[2], s));
  HIP_TRY(hipMemcpyAsync(st->totals, st->d_totals, sizeof(st->totals), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 2; k++) HIP_TRY(st->block.elapsed_ms(k, &st->kernel_ms[k]));
  st->prev_mid = cfg->prev_mid;
  st->deltat = cfg->deltat;
  st->nprocs = cfg->nprocs;
  st->lte = a.lte;
  st->valid = true;
  st->serial++;
  e->fit_since_step = true;
  return ARTIS_OK;
}

int artis_amd_radfield_download(artis_amd_engine *e, artis_radfield *out) {
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "radfield: null argument");
  STAGE_STRUCT_SIZE(out, artis_radfield, "radfield");
  if (!e->rf || !e->rf->valid) return stage_error(ARTIS_ERR_ARG, "radfield: nothing fitted (artis_amd_radfield_fit)");
  RfState *st = e->rf;
  if (((out->radfieldbin_T_R || out->radfieldbin_W) && st->nbins == 0) || (out->bfrate_normed && st->nbf == 0) ||
      ((out->Jb_lu_normed || out->Jb_lu_contribcount) && st->nline == 0))
    return stage_error(ARTIS_ERR_ARG, "radfield: an array was asked for that this build does not make");
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->ncell;
  HIP_TRY(stage_copy(out->J, st->d_J, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->nuJ, st->d_nuJ, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->J_normfactor, st->d_normfactor, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->TJ, st->d_TJ, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->TR, st->d_TR, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->Te, st->d_Te, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->W, st->d_W, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->flags, st->d_flags, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->cell_counts, st->d_counts, n * ARTIS_RADFIELD_NCOUNTS, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->radfieldbin_T_R, st->d_bin_T_R, n * st->nbins, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->radfieldbin_W, st->d_bin_W, n * st->nbins, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->bfrate_normed, st->d_bf, n * st->nbf, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(out->Jb_lu_normed, st->d_Jb, n * st->nline, hipMemcpyDeviceToHost));
  if (out->Jb_lu_contribcount && st->nline > 0) {
    std::vector<double> cnt((size_t)(n * st->nline));
    HIP_TRY(stage_copy(cnt.data(), st->d_Jbcount, n * st->nline, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cnt.size(); i++) out->Jb_lu_contribcount[i] = (int64_t)cnt[i];
  }
  for (int k = 0; k < ARTIS_RADFIELD_NCOUNTS; k++) out->totals[k] = (int64_t)st->totals[k];
  out->npts_nonempty = (int32_t)n;
  out->nbins = (int32_t)st->nbins;
  out->nbfestim = (int32_t)st->nbf;
  out->detailed_linecount = (int32_t)st->nline;
  out->kernel_ms[0] = st->kernel_ms[0];
  out->kernel_ms[1] = st->kernel_ms[1];
  return ARTIS_OK;
}

}  // extern "C"
