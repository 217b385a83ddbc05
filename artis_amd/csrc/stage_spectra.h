// stage_spectra.h -- artis_amd_spectra_*: spectra and light curves of the resident packets (rules: spectra.h).
// Every output element is the sequential sum of its contributions in the caller's packet order, whatever slots the packets
// sit in and in whatever order the threads run. k_spec_prep first brings the packets into caller order (the SpecPkt of caller
// packet perm[slot] from record slot); then per family of outputs (spectra.h SpecFamily):
//   k_spec_keys      entry e -> key = output element (or the sentinel: no contribution), value = e; entries are in caller order
//   radix sort       (rocPRIM, stable): the entries of one element side by side, still in caller order
//   k_spec_heads     the first entry of every element's run
// and per array of the family (I, Q, U):
//   k_spec_values    the contribution of every sorted entry, side by side in sorted order
//   k_spec_runsum    one wave per run: the lanes load the run 512 entries at a time (the next 512 while the current ones are
//                    added), and every lane adds them in order (v_readlane), so each lane holds the same sequential sum.
#pragma once

namespace {

__global__ void __launch_bounds__(BLOCK) k_spec_prep(PktStore P, const int32_t *perm, artis_spec::SpecRules R, artis_spec::SpecPkt *out,
                                                    unsigned long long *counts) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int kind = 0;
  if (i < P.n) {
    artis_packet a;
    rec_to_aos(P, i, a);
    const artis_spec::SpecPkt s = artis_spec::classify(a, R);
    out[perm ? perm[i] : i] = s;
    kind = s.kind;
  }
  // escaped r-packets and gamma packets: one atomic per wave and kind
  const unsigned long long nr = __ballot(kind == 1), ng = __ballot(kind == 2);
  if ((threadIdx.x & 63) == 0) {
    if (nr) atomicAdd(&counts[0], (unsigned long long)__popcll(nr));
    if (ng) atomicAdd(&counts[1], (unsigned long long)__popcll(ng));
  }
}
__global__ void __launch_bounds__(BLOCK) k_spec_bfcols(DevModel M, int max_nions, int32_t *bf_col) {
  const int ui = blockIdx.x * BLOCK + threadIdx.x;
  if (ui >= M.nions) return;
  artis_spec::fill_bf_columns_of_ion(ui, M.ion_element, M.elem_uniqueionindexstart, M.ion_uniquelevelindexstart, M.ion_nlevels_ionising,
                                     M.level_nphixstargets, M.level_bflist_start, max_nions, M.nbfcontinua, bf_col);
}
__global__ void __launch_bounds__(BLOCK) k_spec_keys(const artis_spec::SpecPkt *pk, int64_t n, int64_t nent, int fam, artis_spec::SpecShape S,
                                                    uint32_t sentinel, uint32_t *keys, uint32_t *ents) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= nent) return;
  const int half = e >= n;
  int64_t slot;
  double saf;
  keys[e] = artis_spec::family_entry(fam, S, pk[half ? e - n : e], half, &slot, &saf) ? (uint32_t)slot : sentinel;
  ents[e] = (uint32_t)e;
}
__global__ void __launch_bounds__(BLOCK) k_spec_heads(const uint32_t *keys, int64_t nent, uint32_t sentinel, uint32_t *heads, uint32_t *nheads) {
  const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= nent) return;
  const uint32_t k = keys[j];
  if (k != sentinel && (j == 0 || keys[j - 1] != k)) heads[atomicAdd(nheads, 1u)] = (uint32_t)j;
}
__global__ void __launch_bounds__(BLOCK) k_spec_values(const artis_spec::SpecPkt *pk, int64_t n, artis_spec::SpecRules R, artis_spec::SpecShape S,
                                                      int fam, int comp, const uint32_t *keys, const uint32_t *ents, int64_t nent,
                                                      uint32_t sentinel, double *vals) {
  const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= nent || keys[j] == sentinel) return;  // (k_spec_runsum reads no value of an entry without a contribution)
  const int64_t e = ents[j];
  const int half = e >= n;
  const artis_spec::SpecPkt s = pk[half ? e - n : e];
  int64_t slot;
  double saf;
  (void)artis_spec::family_entry(fam, S, s, half, &slot, &saf);
  vals[j] = artis_spec::family_value(fam, comp, s, R, saf);
}
__device__ inline double readlane_f64(double v, int lane) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
constexpr int SPEC_RUN_K = 8;  // entries per lane per round: 512 per wave
// entries base + k * 64 + lane of a round (order within the round: k-major, lane-minor); past the end: a key that is not `key`
__device__ inline void spec_round_load(const uint32_t *keys, const double *vals, int64_t nent, int64_t base, int lane, uint32_t key,
                                       uint32_t kk[SPEC_RUN_K], double vv[SPEC_RUN_K]) {
#pragma unroll
  for (int k = 0; k < SPEC_RUN_K; k++) {
    const int64_t j = base + k * 64 + lane;
    kk[k] = j < nent ? keys[j] : ~key;
    vv[k] = j < nent ? vals[j] : 0.;
  }
}
__global__ void __launch_bounds__(BLOCK) k_spec_runsum(const uint32_t *keys, const double *vals, int64_t nent, const uint32_t *heads,
                                                      const uint32_t *nheads, double *out) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * (BLOCK / 64);
  const uint32_t nruns = *nheads;
  for (int64_t r = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); r < nruns; r += nwaves) {
    const int64_t j0 = heads[r];
    const uint32_t key = keys[j0];
    uint32_t kk[SPEC_RUN_K], kn[SPEC_RUN_K];
    double vv[SPEC_RUN_K], vn[SPEC_RUN_K];
    spec_round_load(keys, vals, nent, j0, lane, key, kk, vv);
    double s = 0.;
    for (int64_t base = j0;; base += SPEC_RUN_K * 64) {
      int cnt[SPEC_RUN_K];
      bool full = true;
#pragma unroll
      for (int k = 0; k < SPEC_RUN_K; k++) {
        cnt[k] = __popcll(__ballot(kk[k] == key));  // the run's entries are a prefix of the round (keys sorted)
        full = full && cnt[k] == 64;
      }
      if (full) spec_round_load(keys, vals, nent, base + SPEC_RUN_K * 64, lane, key, kn, vn);  // in flight while this round is added
#pragma unroll
      for (int k = 0; k < SPEC_RUN_K; k++) {
        if (cnt[k] == 64) {
#pragma unroll
          for (int l = 0; l < 64; l++) s += readlane_f64(vv[k], l);
        } else {
          for (int l = 0; l < cnt[k]; l++) s += readlane_f64(vv[k], l);
        }
      }
      if (!full) break;
#pragma unroll
      for (int k = 0; k < SPEC_RUN_K; k++) {
        kk[k] = kn[k];
        vv[k] = vn[k];
      }
    }
    if (lane == 0) out[key] = s;
  }
}

// scratch and outputs of artis_amd_spectra_* (allocated at the first call, grown when needed: spec_reserve)
struct SpecState {
  // grown together by spec_reserve(): after a failed allocation all of them are freed and every capacity is 0
  artis_spec::SpecPkt *d_pk = nullptr;  // [pk_cap]
  uint32_t *d_keys = nullptr, *d_keys2 = nullptr, *d_ents = nullptr, *d_ents2 = nullptr, *d_heads = nullptr;  // [ent_cap]
  double *d_vals = nullptr;             // [ent_cap]
  void *d_sort_tmp = nullptr;           // [sort_tmp_bytes]
  double *d_block = nullptr;            // [block_cap]
  double *d_times = nullptr;            // [2 * times_cap] starts, widths
  int64_t pk_cap = 0, ent_cap = 0, block_cap = 0, times_cap = 0;
  size_t sort_tmp_bytes = 0;
  // made once (spec_init)
  unsigned long long *d_counts = nullptr;  // [2] escaped r-packets, gamma packets; then the run count (uint32)
  float *d_grid = nullptr;                 // delta_freq of the r-packet and of the gamma grid
  float h_lower[2][artis_spec::MNUBINS], h_delta[2][artis_spec::MNUBINS];
  artis_spec::SpecGrid grid_r{}, grid_g{};
  int32_t *d_bfcol = nullptr;
  int32_t max_nions = 0;
  // the last compute
  bool valid = false;
  int64_t off[artis_spec::NOUT] = {}, size[artis_spec::NOUT] = {};
  int64_t ndoubles = 0;
  artis_spec::SpecShape shape{};
  unsigned long long counts[2] = {};
};

void spec_free_scratch(SpecState *st) {
  void **ptrs[] = {(void **)&st->d_pk, (void **)&st->d_keys, (void **)&st->d_keys2, (void **)&st->d_ents, (void **)&st->d_ents2,
                   (void **)&st->d_heads, (void **)&st->d_vals, &st->d_sort_tmp, (void **)&st->d_block, (void **)&st->d_times};
  for (void **q : ptrs) {
    if (*q) (void)hipFree(*q);
    *q = nullptr;
  }
  st->pk_cap = st->ent_cap = st->block_cap = st->times_cap = 0;
  st->sort_tmp_bytes = 0;
}

void spec_free(SpecState *st) {
  if (!st) return;
  spec_free_scratch(st);
  void *ptrs[] = {st->d_counts, st->d_grid, st->d_bfcol};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  delete st;
}

int spec_end_bit(uint32_t sentinel) {  // radix-sort bits that hold every key of a family, the sentinel included
  int end_bit = 1;
  while (end_bit < 32 && ((uint64_t)1 << end_bit) <= (uint64_t)sentinel) end_bit++;
  return end_bit;
}
// Scratch for n packets, nent entries, the output block and the time grid. When any of it is too small, all of it is freed and
// allocated anew at the larger of old and new size; when an allocation fails, all of it is freed and every capacity is 0, so that
// no later call finds a capacity without its buffer. The new bytes must fit 90 % of the free device memory (ARTIS_ERR_ARG).
int spec_reserve(SpecState *st, int64_t n, int64_t nent, int64_t ndoubles, int64_t ntimesteps, size_t sort_tmp) {
  if (st->d_pk && st->pk_cap >= n && st->ent_cap >= nent && st->block_cap >= ndoubles && st->times_cap >= ntimesteps &&
      st->sort_tmp_bytes >= sort_tmp)
    return ARTIS_OK;
  const int64_t npk = std::max(st->pk_cap, n), nen = std::max(st->ent_cap, nent), nbl = std::max(st->block_cap, ndoubles),
                nts = std::max(st->times_cap, ntimesteps);
  const size_t ntmp = std::max(st->sort_tmp_bytes, sort_tmp);
  auto bytes = [](int64_t pk, int64_t en, int64_t bl, int64_t ts, size_t tmp) {
    return (double)sizeof(artis_spec::SpecPkt) * pk + (5. * sizeof(uint32_t) + sizeof(double)) * en + (double)sizeof(double) * bl +
           2. * sizeof(double) * ts + (double)tmp;
  };
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const double held = st->d_pk ? bytes(st->pk_cap, st->ent_cap, st->block_cap, st->times_cap, st->sort_tmp_bytes) : 0.;
  if (bytes(npk, nen, nbl, nts, ntmp) - held > 0.9 * (double)free_b)
    return stage_error(ARTIS_ERR_ARG, "spectra: the output arrays and the scratch do not fit the free device memory");
  spec_free_scratch(st);
  auto one = [](int64_t c) { return (size_t)(c > 0 ? c : 1); };
  hipError_t err = hipMalloc((void **)&st->d_pk, sizeof(artis_spec::SpecPkt) * one(npk));
  for (uint32_t **q : {&st->d_keys, &st->d_keys2, &st->d_ents, &st->d_ents2, &st->d_heads})
    if (err == hipSuccess) err = hipMalloc((void **)q, sizeof(uint32_t) * one(nen));
  if (err == hipSuccess) err = hipMalloc((void **)&st->d_vals, sizeof(double) * one(nen));
  if (err == hipSuccess) err = hipMalloc(&st->d_sort_tmp, ntmp > 0 ? ntmp : 1);
  if (err == hipSuccess) err = hipMalloc((void **)&st->d_block, sizeof(double) * one(nbl));
  if (err == hipSuccess) err = hipMalloc((void **)&st->d_times, 2 * sizeof(double) * one(nts));
  if (err != hipSuccess) {
    spec_free_scratch(st);
    g_last_error = std::string("spectra: hipMalloc of the scratch: ") + hipGetErrorString(err);
    return ARTIS_ERR_HIP;
  }
  st->pk_cap = npk;
  st->ent_cap = nen;
  st->block_cap = nbl;
  st->times_cap = nts;
  st->sort_tmp_bytes = ntmp;
  return ARTIS_OK;
}
// once per engine: the frequency grids (init_spectra, on the host as the reference does) and the column maps
int spec_init(artis_amd_engine *e) {
  if (e->spec) return ARTIS_OK;
  SpecState *st = new SpecState();
  e->spec = st;
  using namespace artis_spec;
  st->grid_r = make_grid(ARTIS_OPT_NU_MIN_R, ARTIS_OPT_NU_MAX_R, st->h_lower[0], st->h_delta[0]);
  st->grid_g = make_grid(NU_MIN_GAMMA, NU_MAX_GAMMA, st->h_lower[1], st->h_delta[1]);
  HIP_TRY(hipMalloc((void **)&st->d_grid, sizeof(float) * 2 * MNUBINS));
  HIP_TRY(hipMemcpy(st->d_grid, st->h_delta[0], sizeof(float) * MNUBINS, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(st->d_grid + MNUBINS, st->h_delta[1], sizeof(float) * MNUBINS, hipMemcpyHostToDevice));
  st->grid_r.delta_freq = st->d_grid;
  st->grid_g.delta_freq = st->d_grid + MNUBINS;
  HIP_TRY(hipMalloc((void **)&st->d_counts, sizeof(unsigned long long) * 4));
  std::vector<int32_t> nions(e->Mh.nelements > 0 ? e->Mh.nelements : 1, 0);
  if (e->Mh.nelements > 0)
    HIP_TRY(hipMemcpy(nions.data(), e->M.elem_nions, sizeof(int32_t) * (size_t)e->Mh.nelements, hipMemcpyDeviceToHost));
  st->max_nions = *std::max_element(nions.begin(), nions.end());
  const int nbf = e->Mh.nbfcontinua;
  HIP_TRY(hipMalloc((void **)&st->d_bfcol, sizeof(int32_t) * (size_t)(nbf > 0 ? nbf : 1)));
  HIP_TRY(hipMemset(st->d_bfcol, 0xFF, sizeof(int32_t) * (size_t)(nbf > 0 ? nbf : 1)));  // -1: an entry no level fills
  if (e->Mh.nions > 0) {
    hipLaunchKernelGGL(k_spec_bfcols, dim3(nblocks(e->Mh.nions)), dim3(BLOCK), 0, nullptr, e->M, st->max_nions, st->d_bfcol);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipDeviceSynchronize());
  return ARTIS_OK;
}
}  // namespace

extern "C" {

int artis_amd_spectra_compute(artis_amd_engine *e, const artis_spectra_config *cfg, void *hip_stream) {
  using namespace artis_spec;
  if (!e || !cfg) return stage_error(ARTIS_ERR_ARG, "spectra: null engine or config");
  STAGE_STRUCT_SIZE(cfg, artis_spectra_config, "spectra");
  if (cfg->ntimesteps < 1) return stage_error(ARTIS_ERR_ARG, "spectra: ntimesteps < 1");
  if (!cfg->ts_start || !cfg->ts_width) return stage_error(ARTIS_ERR_ARG, "spectra: null ts_start or ts_width");
  for (int i = 1; i < cfg->ntimesteps; i++)
    if (!(cfg->ts_start[i] > cfg->ts_start[i - 1])) return stage_error(ARTIS_ERR_ARG, "spectra: timestep starts do not increase");
  if (!(cfg->dirbin == -1 || cfg->dirbin == ARTIS_SPEC_ALL_DIRBINS || (cfg->dirbin >= 0 && cfg->dirbin < MABINS)))
    return stage_error(ARTIS_ERR_ARG, "spectra: dirbin out of range (-1, 0..MABINS-1 or ARTIS_SPEC_ALL_DIRBINS)");
  if (e->npackets < 0 || !e->d_pkt) return stage_error(ARTIS_ERR_ARG, "spectra: no resident packets");
  HIP_TRY(hipSetDevice(e->device));
  int rc = spec_init(e);
  if (rc != ARTIS_OK) {
    spec_free(e->spec);
    e->spec = nullptr;
    return rc;
  }
  SpecState *st = e->spec;
  st->valid = false;
  hipStream_t s = (hipStream_t)hip_stream;

  SpecShape S{};
  S.dirbin = cfg->dirbin;
  S.ndirslots = cfg->dirbin == ARTIS_SPEC_ALL_DIRBINS ? 1 + MABINS : 1;
  S.ntimesteps = cfg->ntimesteps;
  S.nabscols = e->Mh.nelements * st->max_nions;
  S.proccount = 2 * S.nabscols + 1;
  S.emission_absorption = cfg->emission_absorption != 0;
  S.stokes = cfg->stokes != 0;
  S.gamma = cfg->gamma != 0;
  // the output block, and the keys: an output element's index must fit 32 bits beside the sentinel
  int64_t ndoubles = 0;
  for (int o = 0; o < NOUT; o++) st->size[o] = 0;
  for (int fam = 0; fam < NFAM; fam++) {
    if (!family_on(fam, S)) continue;
    const int64_t sz = family_size(fam, S);
    if (sz >= (int64_t)0xFFFFFFFFLL)
      return stage_error(ARTIS_ERR_ARG, S.ndirslots > 1 ? "spectra: the arrays of all direction bins do not fit 32-bit indices (emission_absorption)"
                                            : "spectra: the arrays do not fit 32-bit indices");
    for (int c = 0; c < family_ncomp(fam, S); c++) st->size[family_output(fam, c)] = sz;
  }
  for (int o = 0; o < NOUT; o++) {
    st->off[o] = ndoubles;
    ndoubles += st->size[o];
  }
  const int64_t n = e->npackets;
  const int64_t nent = n * (S.ndirslots > 1 ? 2 : 1);
  if (nent >= (int64_t)0xFFFFFFFFLL) return stage_error(ARTIS_ERR_ARG, "spectra: too many packets for 32-bit entry indices");
  size_t sort_tmp = 0;  // the largest rocPRIM scratch of the families (a size query: no buffer is touched)
  for (int fam = 0; fam < NFAM; fam++) {
    if (!family_on(fam, S)) continue;
    size_t tmp = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                      (size_t)nent, 0, spec_end_bit((uint32_t)family_size(fam, S)), s));
    sort_tmp = std::max(sort_tmp, tmp);
  }
  rc = spec_reserve(st, n, nent, ndoubles, cfg->ntimesteps, sort_tmp);
  if (rc != ARTIS_OK) return rc;
  HIP_TRY(hipMemcpyAsync(st->d_times, cfg->ts_start, sizeof(double) * (size_t)cfg->ntimesteps, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(st->d_times + cfg->ntimesteps, cfg->ts_width, sizeof(double) * (size_t)cfg->ntimesteps, hipMemcpyHostToDevice, s));

  SpecRules R{};
  R.T.ntimesteps = cfg->ntimesteps;
  R.T.start = st->d_times;
  R.T.width = st->d_times + cfg->ntimesteps;
  R.T.tmin = cfg->tmin;
  R.T.tmax = cfg->tmax;
  R.r = st->grid_r;
  R.g = st->grid_g;
  R.cols.nelements = e->Mh.nelements;
  R.cols.max_nions = st->max_nions;
  R.cols.nlines = e->Mh.nlines;
  R.cols.nbfcontinua = e->Mh.nbfcontinua;
  R.cols.line_elementindex = e->M.line_elementindex;
  R.cols.line_ionindex = e->M.line_ionindex;
  R.cols.bf_col = st->d_bfcol;
  R.inverse_gamma = std::sqrt(1. - (e->model_copy.vmax * e->model_copy.vmax / (artis_spec::CLIGHT * artis_spec::CLIGHT)));  // :703
  R.want_columns = S.emission_absorption;

  HIP_TRY(hipMemsetAsync(st->d_block, 0, sizeof(double) * (size_t)(ndoubles > 0 ? ndoubles : 1), s));
  HIP_TRY(hipMemsetAsync(st->d_counts, 0, sizeof(unsigned long long) * 4, s));
  if (n > 0) {
    hipLaunchKernelGGL(k_spec_prep, dim3(nblocks(n)), dim3(BLOCK), 0, s, e->P, e->use_perm ? e->d_perm : nullptr, R, st->d_pk, st->d_counts);
    HIP_TRY(hipGetLastError());
    uint32_t *nheads = (uint32_t *)(st->d_counts + 2);
    for (int fam = 0; fam < NFAM; fam++) {
      if (!family_on(fam, S)) continue;
      const uint32_t sentinel = (uint32_t)family_size(fam, S);
      const int end_bit = spec_end_bit(sentinel);
      hipLaunchKernelGGL(k_spec_keys, dim3(nblocks(nent)), dim3(BLOCK), 0, s, st->d_pk, n, nent, fam, S, sentinel, st->d_keys, st->d_ents);
      HIP_TRY(hipGetLastError());
      size_t tmp = st->sort_tmp_bytes;
      HIP_TRY(rocprim::radix_sort_pairs(st->d_sort_tmp, tmp, st->d_keys, st->d_keys2, st->d_ents, st->d_ents2, (size_t)nent, 0, end_bit, s));
      HIP_TRY(hipMemsetAsync(nheads, 0, sizeof(uint32_t), s));
      hipLaunchKernelGGL(k_spec_heads, dim3(nblocks(nent)), dim3(BLOCK), 0, s, st->d_keys2, nent, sentinel, st->d_heads, nheads);
      HIP_TRY(hipGetLastError());
      for (int c = 0; c < family_ncomp(fam, S); c++) {
        hipLaunchKernelGGL(k_spec_values, dim3(nblocks(nent)), dim3(BLOCK), 0, s, st->d_pk, n, R, S, fam, c, st->d_keys2, st->d_ents2, nent,
                           sentinel, st->d_vals);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_spec_runsum, dim3(2048), dim3(BLOCK), 0, s, st->d_keys2, st->d_vals, nent, st->d_heads, nheads,
                           st->d_block + st->off[family_output(fam, c)]);
        HIP_TRY(hipGetLastError());
      }
    }
  }
  HIP_TRY(hipMemcpyAsync(st->counts, st->d_counts, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  st->ndoubles = ndoubles;
  st->shape = S;
  st->valid = true;
  return ARTIS_OK;
}

int artis_amd_spectra_devptr(artis_amd_engine *e, void **dptr, int64_t *ndoubles) {
  if (!e || !dptr || !ndoubles) return stage_error(ARTIS_ERR_ARG, "spectra: null argument");
  if (!e->spec || !e->spec->valid) return stage_error(ARTIS_ERR_ARG, "spectra: nothing computed (artis_amd_spectra_compute)");
  *dptr = e->spec->d_block;
  *ndoubles = e->spec->ndoubles;
  return ARTIS_OK;
}

int artis_amd_spectra_download(artis_amd_engine *e, artis_spectra *out) {
  using namespace artis_spec;
  if (!e || !out) return stage_error(ARTIS_ERR_ARG, "spectra: null argument");
  STAGE_STRUCT_SIZE(out, artis_spectra, "spectra");
  if (!e->spec || !e->spec->valid) return stage_error(ARTIS_ERR_ARG, "spectra: nothing computed (artis_amd_spectra_compute)");
  SpecState *st = e->spec;
  double *dst[NOUT] = {out->lum, out->lumcmf, out->flux, out->flux_q, out->flux_u, out->emission, out->emission_q, out->emission_u,
                       out->trueemission, out->absorption, out->absorption_q, out->absorption_u, out->gamma_lum, out->gamma_lumcmf,
                       out->gamma_flux};
  for (int o = 0; o < NOUT; o++)
    if (dst[o] && st->size[o] == 0) return stage_error(ARTIS_ERR_ARG, "spectra: an array was asked for that the last compute did not produce");
  HIP_TRY(hipSetDevice(e->device));
  for (int o = 0; o < NOUT; o++)
    if (dst[o]) HIP_TRY(hipMemcpy(dst[o], st->d_block + st->off[o], sizeof(double) * (size_t)st->size[o], hipMemcpyDeviceToHost));
  if (out->lower_freq) std::memcpy(out->lower_freq, st->h_lower[0], sizeof(float) * MNUBINS);
  if (out->delta_freq) std::memcpy(out->delta_freq, st->h_delta[0], sizeof(float) * MNUBINS);
  if (out->gamma_lower_freq) std::memcpy(out->gamma_lower_freq, st->h_lower[1], sizeof(float) * MNUBINS);
  if (out->gamma_delta_freq) std::memcpy(out->gamma_delta_freq, st->h_delta[1], sizeof(float) * MNUBINS);
  out->nescaped_rpkt = (int64_t)st->counts[0];
  out->nescaped_gamma = (int64_t)st->counts[1];
  out->ntimesteps = st->shape.ntimesteps;
  out->ndirslots = st->shape.ndirslots;
  out->nelements = e->Mh.nelements;
  out->max_nions = st->max_nions;
  out->proccount = st->shape.proccount;
  return ARTIS_OK;
}

}  // extern "C"
