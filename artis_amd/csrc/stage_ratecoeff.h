// stage_ratecoeff.h -- artis_amd_ratecoeff_*: the rate-coefficient tables on the device (rules and bodies: ratecoeff_tables.h).
// One kernel on the null stream, k_rc_tables: one lane per (continuum, temperature), temperature fastest, so the lanes of a wave share a
// continuum (or two): the abscissae of the two first nodes and the cross-section there are the same for all of them, and only the
// exponentials differ from lane to lane. A workgroup therefore stages the cross-sections of the continua its lanes touch at the two
// sets of 61 abscissae in LDS (at most RC_MAXC continua), and a lane's first nodes read them by node index: alpha_sp and bfcooling from
// one set of evaluations, gammacorr from its own (ratecoeff_tables.h rc_entry_shared_with). An integral whose first node asks to
// subdivide goes through gk61_integrate on the table itself. Launched in batches of items_per_launch entries: no launch's length
// depends on the data set. Every element of the tables and flags has one writer; the totals are integers, summed per wave behind one
// ballot each and added by the wave's first lane.
#pragma once

namespace {

constexpr int64_t RC_ITEMS_PER_LAUNCH = (int64_t)1 << 20;
constexpr int RC_MAXC = (BLOCK - 1) / artis_rc::TABLESIZE + 2;  // continua the items of one workgroup can touch
constexpr int RC_NSETS = ARTIS_OPT_USE_LUT_PHOTOION ? 2 : 1;    // abscissa sets: nu - nu_edge (alpha_sp, bfcooling) and nu (gammacorr)

struct RcArgs {
  artis::DevModel M;
  artis_rc::Arrays A;
  int64_t item0;   // the launch's first item
  int64_t nitems;  // ... and how many it takes
  unsigned long long *totals;
};

// the cross-section at a node of the lane's continuum, staged by the workgroup
struct RcSigmaStaged {
  const float *sets;  // [RC_NSETS][NSLOTS]
  __device__ float alpha_cooling(const int slot, const double) const { return sets[slot]; }
  __device__ float gammacorr(const int slot, const double) const { return sets[artis_rc::NSLOTS + slot]; }
};

__global__ void __launch_bounds__(BLOCK) k_rc_tables(RcArgs a) {
  __shared__ float staged[RC_MAXC * RC_NSETS * artis_rc::NSLOTS];
  constexpr int PER_CONT = RC_NSETS * artis_rc::NSLOTS;
  const int64_t first = (int64_t)blockIdx.x * BLOCK;  // within the launch
  const int64_t last = (first + BLOCK < a.nitems ? first + BLOCK : a.nitems) - 1;
  const int64_t c_lo = (a.item0 + first) / artis_rc::TABLESIZE;
  const int ncont = (int)((a.item0 + last) / artis_rc::TABLESIZE - c_lo) + 1;  // <= RC_MAXC: last - first < BLOCK
  for (int k = threadIdx.x; k < ncont * PER_CONT; k += BLOCK) {
    const int cl = k / PER_CONT, r = k - cl * PER_CONT;
    const artis_rc::Cont cont = a.A.conts[c_lo + cl];
    if (cont.ul < 0) continue;  // (no lane reads the row's values)
    const artis_rc::ContConsts kc = artis_rc::cont_consts(a.M, cont);
    const int slot = r % artis_rc::NSLOTS;
    staged[k] = (r < artis_rc::NSLOTS)
                    ? kc.grid.at(kc.nu_threshold, artis_rc::rc_abscissa(slot, 0, kc.nu_max_phixs - kc.nu_threshold) + kc.nu_threshold)
                    : kc.grid.at(kc.nu_threshold, artis_rc::rc_abscissa(slot, kc.nu_threshold, kc.nu_max_phixs));
  }
  __syncthreads();
  const int64_t i = first + threadIdx.x;
  artis_rc::Totals tot{};
  if (i < a.nitems) {
    const int64_t item = a.item0 + i;
    const int64_t ci = item / artis_rc::TABLESIZE;
    const artis_rc::Cont cont = a.A.conts[ci];
    double v[3] = {0., 0., 0.};
    int32_t flag = 0;
    if (cont.ul >= 0) {
      const artis_rc::ContConsts kc = artis_rc::cont_consts(a.M, cont);
      const RcSigmaStaged sigma{staged + (int)(ci - c_lo) * PER_CONT};
      flag = artis_rc::rc_entry_shared_with<artis_rc::TbMath>(a.M, a.A.Tpow, kc, sigma, (int)(item - ci * artis_rc::TABLESIZE), v, &tot);
    }
    artis_rc::store_item(a.A, item, v, flag, &tot);
  }
  // the wave's sums of the lanes' totals; every lane of the wave arrives here
  for (int k = 0; k < artis_rc::NTOTALS; k++) {
    long long t = tot.v[k];
    if (__ballot(t != 0) == 0) continue;  // (wave-uniform)
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&a.totals[k], (unsigned long long)t);
  }
}

// everything of artis_amd_ratecoeff_*: one block, made at the first call
struct RcState {
  StageBlock block;
  int64_t nbf = 0, nitems = 0, ncovered = 0;
  double *d_spont = nullptr, *d_gamma = nullptr, *d_cool = nullptr, *d_Tpow = nullptr;
  int32_t *d_flags = nullptr;
  artis_rc::Cont *d_conts = nullptr;
  unsigned long long *d_totals = nullptr;
  bool valid = false;
  unsigned long long totals[artis_rc::NTOTALS] = {};
  int64_t flagged = 0, first_flagged = -1;
  double kernel_ms = 0.;
};

void rc_free(RcState *st) { delete st; }

int rc_init(artis_amd_engine *e) {
  if (e->rc) return ARTIS_OK;
  const DevModel &h = e->Mh;
  const int64_t nbf = h.nbfcontinua;
  // the index arrays of the reference's loops and the temperature grid, from the device's copies
  auto fetch = [&](const int32_t *dev, int64_t count, std::vector<int32_t> &to) -> hipError_t {
    to.assign((size_t)(count > 0 ? count : 1), 0);
    return count > 0 ? hipMemcpy(to.data(), dev, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost) : hipSuccess;
  };
  std::vector<int32_t> elem_nions, elem_start, ion_nionising, ion_lstart, level_nt, level_bfstart, level_xsstart;
  std::vector<double> tgrid((size_t)artis_rc::TABLESIZE + 1), Tpow((size_t)artis_rc::TABLESIZE);
  hipError_t err = fetch(e->M.elem_nions, h.nelements, elem_nions);
  if (err == hipSuccess) err = fetch(e->M.elem_uniqueionindexstart, h.nelements, elem_start);
  if (err == hipSuccess) err = fetch(e->M.ion_nlevels_ionising, h.nions, ion_nionising);
  if (err == hipSuccess) err = fetch(e->M.ion_uniquelevelindexstart, h.nions, ion_lstart);
  if (err == hipSuccess) err = fetch(e->M.level_nphixstargets, h.nlevels, level_nt);
  if (err == hipSuccess) err = fetch(e->M.level_bflist_start, h.nlevels, level_bfstart);
  if (err == hipSuccess) err = fetch(e->M.level_phixsstart, h.nlevels, level_xsstart);
  if (err == hipSuccess) err = hipMemcpy(tgrid.data(), e->M.temperature_grid, sizeof(double) * tgrid.size(), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("ratecoeff_compute: the model's index arrays: ") + hipGetErrorString(err));
  std::vector<artis_rc::Cont> conts;
  if (!artis_rc::list_continua(h.nelements, nbf, e->model_copy.nphixslevels, elem_nions.data(), elem_start.data(), ion_nionising.data(), ion_lstart.data(),
                               level_nt.data(), level_bfstart.data(), level_xsstart.data(), conts))
    return stage_error(ARTIS_ERR_ARG, "ratecoeff_compute: a level's level_bflist_start + target lies outside [0, nbfcontinua), or an ionising level has no cross-section table");
  artis_rc::make_tpow(tgrid.data(), Tpow.data());
  RcState *st = new RcState();
  st->nbf = nbf;
  st->nitems = nbf * artis_rc::TABLESIZE;
  for (const artis_rc::Cont &c : conts) st->ncovered += c.ul >= 0;
  const int rc = st->block.make({piece(&st->d_spont, st->nitems), piece(&st->d_gamma, ARTIS_OPT_USE_LUT_PHOTOION ? st->nitems : 0), piece(&st->d_cool, st->nitems),
                                 piece(&st->d_Tpow, artis_rc::TABLESIZE), piece(&st->d_flags, st->nitems), piece(&st->d_conts, nbf),
                                 piece(&st->d_totals, artis_rc::NTOTALS)},
                                "ratecoeff_compute", "the tables' block");
  if (rc != ARTIS_OK) {
    delete st;
    return rc;
  }
  err = stage_copy(st->d_Tpow, Tpow.data(), artis_rc::TABLESIZE, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = stage_copy(st->d_conts, conts.data(), nbf, hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    delete st;
    return stage_error(ARTIS_ERR_HIP, std::string("ratecoeff_compute: the list of continua: ") + hipGetErrorString(err));
  }
  e->rc = st;
  return ARTIS_OK;
}

}  // namespace

extern "C" {

int artis_amd_ratecoeff_compute(artis_amd_engine *e, const artis_ratecoeff_request *req) {
  if (!e || !req) return stage_error(ARTIS_ERR_ARG, "ratecoeff_compute: null engine or request");
  STAGE_STRUCT_SIZE(req, artis_ratecoeff_request, "ratecoeff_compute");
  if (req->install != 0 && req->install != 1) return stage_error(ARTIS_ERR_ARG, "ratecoeff_compute: install must be 0 or 1");
  if (req->items_per_launch < 0) return stage_error(ARTIS_ERR_ARG, "ratecoeff_compute: items_per_launch must not be negative");
  if (req->install) {  // the set-up phase only: nothing derived from the tables exists yet
    if (e->cellstate_serial != 0)
      return stage_error(ARTIS_ERR_ARG, "ratecoeff_compute: install after a cell state was set (artis_amd_set_cellstate or a hand-over): the cell cache is derived from the tables");
    if (e->ib && e->ib->have_alpha_sp)
      return stage_error(ARTIS_ERR_ARG, "ratecoeff_compute: install after the ion balance made ion_alpha_sp from the tables");
  }
  HIP_TRY(hipSetDevice(e->device));
  int rc = rc_init(e);
  if (rc != ARTIS_OK) return rc;
  RcState *st = e->rc;
  st->valid = false;
  hipStream_t s = nullptr;
  const int64_t n = st->nitems;
  const int64_t per_launch = req->items_per_launch > 0 ? req->items_per_launch : RC_ITEMS_PER_LAUNCH;
  RcArgs a{};
  a.M = e->M;
  a.A.nitems = n;
  a.A.conts = st->d_conts;
  a.A.Tpow = st->d_Tpow;
  a.A.spontrecomb = st->d_spont;
  a.A.corrphotoion = st->d_gamma;
  a.A.bfcooling = st->d_cool;
  a.A.flags = st->d_flags;
  a.totals = st->d_totals;
  HIP_TRY(hipMemsetAsync(st->d_totals, 0, sizeof(unsigned long long) * artis_rc::NTOTALS, s));
  HIP_TRY(hipEventRecord(st->block.ev[0], s));
  for (int64_t i0 = 0; i0 < n; i0 += per_launch) {
    a.item0 = i0;
    a.nitems = std::min(per_launch, n - i0);
    hipLaunchKernelGGL(k_rc_tables, dim3(nblocks(a.nitems)), dim3(BLOCK), 0, s, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("ratecoeff_compute: k_rc_tables: ") + hipGetErrorString(err));
  }
  HIP_TRY(hipEventRecord(st->block.ev[1], s));
  std::vector<int32_t> flags((size_t)(n > 0 ? n : 1));
  HIP_TRY(hipMemcpyAsync(st->totals, st->d_totals, sizeof(st->totals), hipMemcpyDeviceToHost, s));
  HIP_TRY(stage_copy(flags.data(), st->d_flags, n, hipMemcpyDeviceToHost, &s));
  {
    const hipError_t err = hipStreamSynchronize(s);
    if (err != hipSuccess) return stage_error(ARTIS_ERR_HIP, std::string("ratecoeff_compute: k_rc_tables: ") + hipGetErrorString(err));
  }
  HIP_TRY(st->block.elapsed_ms(0, &st->kernel_ms));
  st->flagged = 0;
  st->first_flagged = -1;
  for (int64_t i = 0; i < n; i++)
    if (flags[(size_t)i] != 0 && st->flagged++ == 0) st->first_flagged = i;
  st->valid = true;
  if (st->flagged > 0) {
    const int64_t ci = st->first_flagged / artis_rc::TABLESIZE;
    return stage_error(ARTIS_ERR_NOTCONVERGED, "ratecoeff_compute: " + std::to_string(st->flagged) + " entries are negative or not finite, the first at continuum " +
                                                   std::to_string(ci) + ", temperature index " + std::to_string(st->first_flagged - ci * artis_rc::TABLESIZE) +
                                                   " (flags " + std::to_string(flags[(size_t)st->first_flagged]) + "): nothing is installed");
  }
  if (req->install) {  // over the model's tables in place: no pointer changes
    HIP_TRY(stage_copy(e->M.spontrecombcoeffs, st->d_spont, n, hipMemcpyDeviceToDevice, &s));
    if (ARTIS_OPT_USE_LUT_PHOTOION) HIP_TRY(stage_copy(e->M.corrphotoioncoeffs, st->d_gamma, n, hipMemcpyDeviceToDevice, &s));
    HIP_TRY(stage_copy(e->M.bfcooling_coeffs, st->d_cool, n, hipMemcpyDeviceToDevice, &s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return ARTIS_OK;
}

int artis_amd_ratecoeff_download(artis_amd_engine *e, double *spont, double *corrphotoion, double *bfcooling, int32_t *flags, artis_ratecoeff_stats *stats) {
  if (!e) return stage_error(ARTIS_ERR_ARG, "ratecoeff_download: null engine");
  if (stats) STAGE_STRUCT_SIZE(stats, artis_ratecoeff_stats, "ratecoeff_download");
  if (corrphotoion && !ARTIS_OPT_USE_LUT_PHOTOION)
    return stage_error(ARTIS_ERR_ARG, "ratecoeff_download: this build has no USE_LUT_PHOTOION: there is no corrphotoioncoeffs table (pass NULL)");
  if (!e->rc || !e->rc->valid) return stage_error(ARTIS_ERR_ARG, "ratecoeff_download: nothing computed (artis_amd_ratecoeff_compute)");
  RcState *st = e->rc;
  HIP_TRY(hipSetDevice(e->device));
  const int64_t n = st->nitems;
  HIP_TRY(stage_copy(spont, st->d_spont, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(corrphotoion, st->d_gamma, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(bfcooling, st->d_cool, n, hipMemcpyDeviceToHost));
  HIP_TRY(stage_copy(flags, st->d_flags, n, hipMemcpyDeviceToHost));
  if (stats) {
    stats->integrals = (int64_t)st->totals[0];
    stats->nodes = (int64_t)st->totals[1];
    stats->at_depth_cap = (int64_t)st->totals[2];
    stats->flagged = st->flagged;
    stats->first_flagged = st->first_flagged;
    stats->nbfcontinua = st->nbf;
    stats->ncovered = st->ncovered;
    stats->tablesize = artis_rc::TABLESIZE;
    stats->ntables = ARTIS_OPT_USE_LUT_PHOTOION ? 3 : 2;
    stats->kernel_ms = st->kernel_ms;
  }
  return ARTIS_OK;
}

}  // extern "C"
