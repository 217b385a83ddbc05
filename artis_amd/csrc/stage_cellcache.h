// stage_cellcache.h -- the host's side of the cell cache: filling rows (the kernels of cellcache_kernels.h), making cells resident in a tiled
// cache (the decisions are cache_residency.h's; here are the copies and the fills they ask for), and the entry points that populate, describe
// and inspect the cache. The sizing of the rows stays with engine_fill, which artis_amd_engine_plan shares.
#pragma once
#include "cellcache_view.h"
namespace {
// ---- populate_tile()'s steps
// The pool of on-demand records: a fill of the whole cache empties it. A fill of some cells of a tiled cache leaves it alone -- the cells that stay
// resident keep their cold levels' records; the rows that are filled start without any (k_ma_reset of launch_fill_batch), and the units the cells before
// them held stay handed out until the pool is used up and emptied (reset_pool_if_due() of the propagation loop), which costs fills, never an answer.
// ARTIS_AMD_POOL_KEEP=0: emptied with every fill (round 5). (Emptying it only with the fills that replace half of the rows or more -- when most of what
// it holds belongs to cells that leave -- was measured too: no better, 1520 against 1498 ms at a quarter of the cache; profiles/r06/tiling.md.)
int empty_pool_for_fill(artis_amd_engine *e, hipStream_t s, bool listed_cells) {
  const DevModel &h = e->Mh;
  if (h.ncold > 0 && (!listed_cells || !e->cc.pool_keep)) {
    HIP_TRY(hipMemsetAsync(e->K.ma_pool_used, 0, sizeof(uint32_t), s));
    if (listed_cells) HIP_TRY(hipMemsetAsync(e->K.ma_rowtab, 0xFF, sizeof(int32_t) * (size_t)(e->cc.res.tile_cells * (int64_t)h.ncold), s));
  }
  return ARTIS_OK;
}
// the kernels of one batch: `ncell` cells, which env describes as the kernels' whole fill (fill_count / fill_cell)
void launch_fill_batch(artis_amd_engine *e, hipStream_t s, const Env &env, int64_t ncell) {
  const DevModel &h = e->Mh;
  if (h.ncold > 0) hipLaunchKernelGGL(k_ma_reset, dim3(nblocks(ncell * h.ncold)), dim3(BLOCK), 0, s, env);
  hipLaunchKernelGGL(k_levelpops, dim3(nblocks(ncell * h.nlevels)), dim3(BLOCK), 0, s, env);
  if (env.ion_absent != nullptr) hipLaunchKernelGGL(k_ion_absent, dim3(nblocks(ncell * 64)), dim3(BLOCK), 0, s, env);  // (tables.h "ABSENT IONS")
  if (h.ndpop > 0) hipLaunchKernelGGL(k_line_dpop, dim3(nblocks(ncell * h.nlines)), dim3(BLOCK), 0, s, env);
  hipLaunchKernelGGL(k_cell_scalars, dim3(nblocks(ncell)), dim3(BLOCK), 0, s, env);
  if (h.nbfcontinua > 0) hipLaunchKernelGGL(k_allcont, dim3(nblocks(ncell * h.nkeepwords * 64)), dim3(BLOCK), 0, s, env);
  if (h.nbfcontinua > 0) hipLaunchKernelGGL(k_keptlist, dim3(nblocks(ncell * 64)), dim3(BLOCK), 0, s, env);
  if (h.nphixstargets_total > 0)
    hipLaunchKernelGGL(k_corrphotoion, dim3(nblocks(ncell * h.nphixstargets_total)), dim3(BLOCK), 0, s, env, e->d_target_level);
  if (h.nalltrans > 0) hipLaunchKernelGGL(k_matrans, dim3(nblocks(ncell * h.nscanblk * 64)), dim3(BLOCK), 0, s, env);
  if (h.nrecomblevels > 0) hipLaunchKernelGGL(k_macroatom_recomb, dim3(nblocks(ncell * (int64_t)h.nrecomblevels * 16)), dim3(BLOCK), 0, s, env);
  hipLaunchKernelGGL(k_macroatom, dim3(nblocks(ncell * h.nlevels)), dim3(BLOCK), 0, s, env);
  if (h.nmalongsegs > 0) hipLaunchKernelGGL(k_mafilter_long, dim3(nblocks(ncell * (int64_t)h.nmalongsegs * 64)), dim3(BLOCK), 0, s, env);
#if ARTIS_EXPOPAC_TABLES
  if (e->expopac_own) {  // needs line_dpop and chi_ff_nnionpart of the batch's cells (k_line_dpop, k_cell_scalars above)
    hipLaunchKernelGGL(k_expopac, dim3(nblocks((int64_t)ncell * ARTIS_EXPOPAC_NBINS)), dim3(BLOCK), 0, s, env);
    if (ARTIS_OPT_RPKT_BB_THERMALISATION) hipLaunchKernelGGL(k_expopac_planck, dim3(nblocks(ncell)), dim3(BLOCK), 0, s, env);
  }
#endif
  hipLaunchKernelGGL(k_cooling_head, dim3(nblocks((int64_t)ncell * h.nions)), dim3(BLOCK), 0, s, env);
  hipLaunchKernelGGL(k_cooling_chain, dim3(nblocks((int64_t)ncell * h.nions * 16)), dim3(BLOCK), 0, s, env);
  if (h.ncoollines > 0) hipLaunchKernelGGL(k_collexc_filter, dim3(nblocks(ncell * (int64_t)h.ncoollines)), dim3(BLOCK), 0, s, env);
  hipLaunchKernelGGL(k_cooling_tail, dim3(nblocks((int64_t)ncell * h.nions * 16)), dim3(BLOCK), 0, s, env);
  hipLaunchKernelGGL(k_cooling_prefix, dim3(nblocks(ncell)), dim3(BLOCK), 0, s, env);
  if (h.nguide > 0) hipLaunchKernelGGL(k_cool_guide, dim3(nblocks(ncell * h.nguide)), dim3(BLOCK), 0, s, env);
}
// after the last batch: wait, count the fills, report what the kernels flagged; a whole-cache fill is then valid for the current cell state
int finish_fill(artis_amd_engine *e, hipStream_t s, int64_t ncell, bool listed_cells) {
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  // UPDATECELL (stats.h:47): one populate per cell
  unsigned long long add = (unsigned long long)ncell, cur = 0;
  HIP_TRY(hipMemcpy(&cur, e->d_stats + ARTIS_STAT_UPDATECELL, sizeof(cur), hipMemcpyDeviceToHost));
  cur += add;
  HIP_TRY(hipMemcpy(e->d_stats + ARTIS_STAT_UPDATECELL, &cur, sizeof(cur), hipMemcpyHostToDevice));
  if (e->d_absent_counts != nullptr) {
    unsigned long long skipped = 0;
    HIP_TRY(hipMemcpy(&skipped, e->d_absent_counts, sizeof(skipped), hipMemcpyDeviceToHost));
    e->last_absent_skipped = (int64_t)skipped;
    if (e->trace) fprintf(stderr, "[artis_amd] population of %lld cells: %lld static records of absent ions left out\n", (long long)ncell, (long long)skipped);
  }
  int32_t err = 0;
  HIP_TRY(hipMemcpy(&err, e->d_err, sizeof(err), hipMemcpyDeviceToHost));
  if (err != 0) {
    (void)hipMemset(e->d_err, 0, sizeof(int32_t));  // the flag is reported once; the next call starts clean
    g_last_error = "cell cache population raised error flag " + std::to_string(err);
    return ARTIS_ERR_NOTCONVERGED;
  }
  e->cc.tile_valid_lo = listed_cells ? -1 : 0;
  return ARTIS_OK;
}

// populate the cell cache: of every cell (nfill < 0: one tile, row = cell), or of the cells e->cc.d_fill_cells[0..nfill) (a tiled cache: their rows are
// in e->cc.d_krow, make_resident())
int populate_tile(artis_amd_engine *e, hipStream_t s, int64_t nfill = -1) {
  const bool listed_cells = nfill >= 0;
  const int lo = 0, hi = e->Mh.npts_nonempty;
  e->cc.tile_lo = lo;
  e->cc.tile_hi = hi;
  e->cc.tile_valid_lo = -1;
  const Env env_tile = make_env(e);
  const int64_t ncell_fill = listed_cells ? nfill : hi - lo;
  if (ncell_fill <= 0) return ARTIS_OK;
  if (const int rc = empty_pool_for_fill(e, s, listed_cells)) return rc;
  if (e->d_absent_counts != nullptr) HIP_TRY(hipMemsetAsync(e->d_absent_counts, 0, sizeof(unsigned long long), s));  // (the records this population leaves out)
  // in batches of pop_batch cells (the scratch of cooling terms holds that many rows); the kernels of a batch see it as
  // their whole fill: a sub-range of the tile, or a stretch of the list of a sparse fill
  for (int64_t b0 = 0; b0 < ncell_fill; b0 += e->cc.pop_batch) {
    const int64_t ncell = std::min<int64_t>(e->cc.pop_batch, ncell_fill - b0);
    Env env = env_tile;
    if (listed_cells) {
      env.fill_cells = e->cc.d_fill_cells + b0;
      env.nfill = (int32_t)ncell;
    } else {
      env.tile_lo = lo + (int)b0;
      env.tile_hi = lo + (int)(b0 + ncell);
    }
    launch_fill_batch(e, s, env, ncell);
  }
  return finish_fill(e, s, ncell_fill, listed_cells);
}

// a tiled cache: no cell is resident (a new cell state: what the rows hold belongs to the old one)
int forget_rows(artis_amd_engine *e, hipStream_t s) {
  if (e->cc.ntiles <= 1) return ARTIS_OK;
  e->cc.res.reset();
  HIP_TRY(hipMemsetAsync(e->cc.d_krow, 0xFF, sizeof(int32_t) * e->cc.res.krow.size(), s));
  if (e->Mh.ncold > 0) {  // ... and no cold level has a record
    HIP_TRY(hipMemsetAsync(e->K.ma_pool_used, 0, sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(e->K.ma_rowtab, 0xFF, sizeof(int32_t) * (size_t)(e->cc.res.tile_cells * (int64_t)e->Mh.ncold), s));
  }
  return ARTIS_OK;
}

// a tiled cache: make the cells want[0..) resident (at most tile_cells of them; Residency::assign gives them rows); the cells that got a row are filled.
// *nfilled: how many that were.
int make_resident(artis_amd_engine *e, const std::vector<int32_t> &want, hipStream_t s, int64_t *nfilled) {
  using artis_residency::Residency;
  Residency &res = e->cc.res;
  *nfilled = 0;
  if (e->cc.ntiles <= 1 || want.empty()) return ARTIS_OK;
  std::vector<int32_t> fresh;
  if (const int err = res.assign(want, fresh)) {
    g_last_error = err == Residency::MORE_CELLS_THAN_ROWS ? "make_resident: more cells than rows" : "make_resident: no row left";
    return ARTIS_ERR_ARG;
  }
  if (fresh.empty()) return ARTIS_OK;
  HIP_TRY(hipMemcpyAsync(e->cc.d_krow, res.krow.data(), sizeof(int32_t) * res.krow.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->cc.d_fill_cells, fresh.data(), sizeof(int32_t) * fresh.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // (fresh is a local)
  const int rc = populate_tile(e, s, (int64_t)fresh.size());
  if (rc != ARTIS_OK) {
    res.give_back(fresh);
    (void)hipMemcpy(e->cc.d_krow, res.krow.data(), sizeof(int32_t) * res.krow.size(), hipMemcpyHostToDevice);
    return rc;
  }
  *nfilled = (int64_t)fresh.size();
  return ARTIS_OK;
}

// the cells that should be resident for the next visit of a tiled run (cache_residency.h choose_cells, with the engine's switches and grid)
void choose_cells(artis_amd_engine *e, const std::vector<int32_t> &waiting, std::vector<int32_t> &want, int64_t *holds, bool *sparse,
                  int64_t win_lo = -1) {
  const DevModel &h = e->Mh;
  const int ndim = (h.gridtype == ARTIS_GRID_SPHERICAL1D) ? 1 : ((h.gridtype == ARTIS_GRID_CYLINDRICAL2D) ? 2 : 3);
  const artis_residency::GridView grid{ndim, h.ncoordgrid, h.coordstride, h.propcell_nonemptymgi, e->cc.h_cell_grid.data()};
  artis_residency::choose_cells(e->cc.res, waiting, h.npts_nonempty, e->cc.tile_block, e->cc.sparse_fill, e->cc.sparse_max_listed, win_lo, grid, want,
                                holds, sparse);
}
// the debug views: the row of cell c, once the cache is filled (one tile) or the cell resident (several)
int debug_row_of(artis_amd_engine *e, int c, int *row) {
  *row = c;
  if (e->cc.ntiles == 1) {  // the cache has to be filled
    if (e->cc.tile_valid_lo != 0) {
      int rc = populate_tile(e, nullptr);
      if (rc != ARTIS_OK) return rc;
    }
  } else {  // the cell has to be resident
    int64_t nfilled = 0;
    int rc = make_resident(e, std::vector<int32_t>{(int32_t)c}, nullptr, &nfilled);
    if (rc != ARTIS_OK) return rc;
    *row = e->cc.res.krow[(size_t)c];  // its row
  }
  return ARTIS_OK;
}
}  // namespace

extern "C" {

int artis_amd_populate_cellcache(artis_amd_engine *e, void *hip_stream) {
  if (!e || !e->have_cells) {
    g_last_error = "no cell state uploaded";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  e->cc.tile_valid_lo = -1;
  // with one tile the whole cache is filled now; with several, artis_amd_update_packets_device() makes cells resident as packets need them
  if (e->cc.ntiles == 1) return populate_tile(e, (hipStream_t)hip_stream);
  return forget_rows(e, (hipStream_t)hip_stream);
}

int artis_amd_cache_tiles(artis_amd_engine *e, int32_t *ntiles, int64_t *cells_per_tile, int64_t *bytes_per_cell) {
  if (!e) return ARTIS_ERR_ARG;
  if (ntiles) *ntiles = e->cc.ntiles;
  if (cells_per_tile) *cells_per_tile = e->cc.res.tile_cells;
  if (bytes_per_cell) *bytes_per_cell = (int64_t)e->cc.cache_bytes_per_cell;
  return ARTIS_OK;
}

int artis_amd_debug_cellcache(artis_amd_engine *e, int c, double *levelpops, double *maprocessrates, double *matrans,
                              double *allcont_nnlevel, double *allcont_departure, double *allcont_edgepart,
                              uint64_t *allcont_keepbits, double *corrphotoioncoeff, double *cooling_contrib,
                              double *ion_cooling_contribs, double *chi_ff_nnionpart) {
  if (!e || !e->have_cells || c < 0 || c >= e->Mh.npts_nonempty) {
    g_last_error = "bad cell index or no cell state";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  const DevModel &h = e->Mh;
  const int cell = c;
  if (const int rc = debug_row_of(e, cell, &c)) return rc;
#define DL(dst, f, T, per)                                                                                            \
  if (dst && (per) > 0) HIP_TRY(hipMemcpy(dst, e->K.f + (int64_t)c * (per), sizeof(T) * (size_t)(per), hipMemcpyDeviceToHost));
  DL(levelpops, levelpops, double, h.nlevels)
  if (maprocessrates || matrans) {
    // the rates from the records; the cumulative sums -- which the records hold as filters only -- re-added on the device from
    // the transitions' terms, the way an undecided draw gets them. A record whose filters are not those of the sequential
    // form fails the call.
    double *d_rates = nullptr, *d_trans = nullptr;
    int32_t *d_bad = nullptr;
    HIP_TRY(hipMalloc((void **)&d_rates, sizeof(double) * (size_t)(h.nlevels * 9 + 1)));
    HIP_TRY(hipMalloc((void **)&d_trans, sizeof(double) * (size_t)(h.nmatransblock + 1)));
    HIP_TRY(hipMalloc((void **)&d_bad, sizeof(int32_t)));
    HIP_TRY(hipMemset(d_bad, 0, sizeof(int32_t)));
    const Env env = make_env(e);
    hipLaunchKernelGGL(k_debug_macache, dim3(nblocks(h.nlevels)), dim3(BLOCK), 0, nullptr, env, cell, d_rates, d_trans, d_bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    int32_t bad = 0;
    HIP_TRY(hipMemcpy(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost));
    if (maprocessrates) HIP_TRY(hipMemcpy(maprocessrates, d_rates, sizeof(double) * (size_t)h.nlevels * 9, hipMemcpyDeviceToHost));
    if (matrans) HIP_TRY(hipMemcpy(matrans, d_trans, sizeof(double) * (size_t)h.nmatransblock, hipMemcpyDeviceToHost));
    (void)hipFree(d_rates);
    (void)hipFree(d_trans);
    (void)hipFree(d_bad);
    if (bad != 0) {
      g_last_error = std::to_string(bad) + " filter entries of the cell's macro-atom records differ from the sequential form";
      return ARTIS_ERR_NOTCONVERGED;
    }
  }
  DL(allcont_nnlevel, allcont_nnlevel, double, h.nbfcontinua)
  DL(allcont_departure, allcont_departure, double, h.nbfcontinua)
  DL(allcont_edgepart, allcont_edgepart, double, h.nbfcontinua)
  if (allcont_keepbits && h.nbfcontinua > 0)  // rows are padded to nkeepwords; the caller's buffer holds ceil(nbfcontinua/64) words
    HIP_TRY(hipMemcpy(allcont_keepbits, e->K.allcont_keepbits + (int64_t)c * h.nkeepwords, sizeof(uint64_t) * (size_t)((h.nbfcontinua + 63) / 64),
                      hipMemcpyDeviceToHost));
  DL(corrphotoioncoeff, corrphotoioncoeff, double, h.nphixstargets_total)
  DL(cooling_contrib, cooling_contrib, double, h.ncoolingterms)
  DL(ion_cooling_contribs, ion_cooling_contribs, double, h.nions)
  DL(chi_ff_nnionpart, chi_ff_nnionpart, double, 1)
#undef DL
  return ARTIS_OK;
}

int artis_amd_debug_cellcache_array(artis_amd_engine *e, int c, int which, void *dst, int64_t dst_bytes, int64_t *written_bytes) {
  if (written_bytes) *written_bytes = 0;
  if (!e || !e->have_cells || c < 0 || c >= e->Mh.npts_nonempty || !dst) {
    g_last_error = "bad cell index, no cell state or no buffer";
    return ARTIS_ERR_ARG;
  }
  CcArrayView v;
  if (!cc_array_view(e->Mh, e->C, e->K, e->expopac_own, which, &v)) {
    g_last_error = "cell-cache array " + std::to_string(which) + " does not exist in this build or model";
    return ARTIS_ERR_ARG;
  }
  const int64_t bytes = (int64_t)v.elem * v.per;
  if (dst_bytes < bytes) {
    if (written_bytes) *written_bytes = bytes;  // (nothing was written: what the row needs)
    g_last_error = "cell-cache array " + std::to_string(which) + ": the row has " + std::to_string((long long)bytes) + " bytes, the buffer " +
                   std::to_string((long long)dst_bytes);
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  int row = c;
  if (const int rc = debug_row_of(e, c, &row)) return rc;
  const int64_t r = v.by_row ? row : c;
  HIP_TRY(hipMemcpy(dst, (const char *)v.base + (r * bytes), (size_t)bytes, hipMemcpyDeviceToHost));
  if (written_bytes) *written_bytes = bytes;
  return ARTIS_OK;
}

}  // extern "C"
