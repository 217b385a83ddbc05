// rpkt_kernels.h -- what the persistent, work-pulling propagation kernels share (work_pull.h, k_launch_reset), k_rpkt, and the kernels that turn its dense
// bound-free estimator rows into the caller's (k_bfest_dense, k_bfrate_expand). Included by artis_engine.hip inside its anonymous namespace.
#pragma once
// ------------------------------------------------------------------ the propagation kernels
// They are PERSISTENT, work-pulling kernels: a lane that has finished with its packet (budget used up, packet handed
// to another list, escaped, end of timestep) immediately takes the next packet of the work list instead of idling
// until the slowest lane of its wave is done. The list is sorted by cell and cut into `nchunks` contiguous chunks with
// one cursor each -- one chunk per WAVE when the list is long enough: a wave then walks its own run of cells, so at any
// time its lanes sit in one or two cells and read the same cell-cache lines. The chunks of the waves of one XCD are
// adjacent (blocks b and b+8 share an XCD, so each XCD's L2 sees one contiguous range of cells). A wave whose chunk is
// used up steals from the other chunks, its own XCD's first. Placement only affects speed, never results.
#ifndef ARTIS_RPKT_WAVES
#define ARTIS_RPKT_WAVES 2
#endif
#ifndef ARTIS_THERMAL_WAVES
#define ARTIS_THERMAL_WAVES 4
#endif
#include "work_pull.h"  // MAX_CHUNKS, Puller, puller_init(), chunk_at(), pull(): handing the list's indices to the waves
// before a launch of the kernel of one kind: its own list's counter, the alternate counter and the chunk cursors (and the flag) start at zero
__global__ void __launch_bounds__(BLOCK) k_launch_reset(int32_t *count, int kind, int32_t *cursors) {
  for (int i = threadIdx.x; i < PULL_SLOTS; i += BLOCK) cursors[i] = 0;
  if (threadIdx.x == 0) {
    count[kind] = 0;
    count[NEXT_NKINDS] = 0;
  }
}
// chunks for a list of n entries consumed by `nwaves` waves: one per wave, fewer when the list is short
inline int chunks_for(int64_t n, int nwaves) {
  int64_t c = std::min<int64_t>(nwaves, n / 128);
  c = std::max<int64_t>(8, (c / 8) * 8);
  return (int)std::min<int64_t>(c, MAX_CHUNKS);
}

#ifndef ARTIS_RPKT_SPLIT_ABSORB
#define ARTIS_RPKT_SPLIT_ABSORB 0  // (1: measured round 5: k_rpkt 265 -> 258 ms, k_slow 16 -> 32 ms, step unchanged, scratch unchanged: off) free-free / bound-free absorptions of r-packets carried out by the slow-path kernel (physics.h PEND_RPKT_ABSORB)
#endif
// r-packets in flight: boundary distance, continuum opacity, line-by-line Sobolev walk, estimators, events.
// CONT_LDS: the static table of bound-free continua (ContPack: edge frequency, target probability, cross-section table,
// ground-continuum index; 32 B per continuum) is copied into LDS once per workgroup and every read of it in the opacity
// sum (rpkt.cc:721, two of the ~five reads per continuum visited) is a ds_read that does not touch the vector L1.
constexpr int CONT_LDS_MAX = 2048;  // continua (64 KB per workgroup, two workgroups per CU)
// LDS accumulators of per-cell estimators for models with few cells (physics.h Env::cellest_lds)
constexpr int RPKT_CELLEST_CAP = 512;      // cells: 3 estimators x 8 B x 512 = 12 KB per workgroup (next to the 64 KB above)
constexpr int RPKT_CELLEST_CAP_NOCONT = 3072;  // ... 72 KB in the kernel form without the continuum table in LDS
constexpr int GAMMA_CELLEST_CAP = 2048;    // cells: 16 KB per workgroup
constexpr int THERMAL_CELLEST_CAP = 4096;  // cells: 32 KB per workgroup, four workgroups per CU
__device__ inline void cellest_begin(Env &env, double *lds, int n, int nthreads, const double *a0, const double *a1 = nullptr,
                                     const double *a2 = nullptr) {
  const int nkinds = a2 ? 3 : (a1 ? 2 : 1);
  for (int i = threadIdx.x; i < n * nkinds; i += nthreads) lds[i] = 0.;
  env.cellest_lds = lds;
  env.cellest_n = n;
  env.cellest_owner[0] = a0;
  env.cellest_owner[1] = a1;
  env.cellest_owner[2] = a2;
}
__device__ inline void scalars_begin(Env &env, double *lds) {
  if (threadIdx.x < ARTIS_NSCALARS) lds[threadIdx.x] = 0.;
  env.scalars_lds = (env.scalars_in_lds && env.E.scalars != nullptr) ? lds : nullptr;
}
__device__ inline void scalars_flush(const Env &env) {  // after a __syncthreads()
  if (env.scalars_lds != nullptr && threadIdx.x < ARTIS_NSCALARS && env.scalars_lds[threadIdx.x] != 0.)
    unsafeAtomicAdd(&env.E.scalars[threadIdx.x], env.scalars_lds[threadIdx.x]);
}
// the estimator form k_thermal<.., TABLES_LDS> takes (its own choice at the top of the kernel): artis_amd_last_estimator_forms
inline int32_t thermal_est_form(const Env &env, int tables_lds) {
  if (env.cellest_n_t > 0) return ARTIS_AMD_EST_THERMAL_LDS;
  return (tables_lds != 2 && env.estcache_on) ? ARTIS_AMD_EST_THERMAL_WAVECACHE : ARTIS_AMD_EST_THERMAL_GLOBAL;
}
// call after a __syncthreads(): the workgroup's sums of one estimator go to the global array
__device__ inline void cellest_flush(const Env &env, int kind, double *global_array, int nthreads) {
  for (int c = threadIdx.x; c < env.cellest_n; c += nthreads) {
    const double v = env.cellest_lds[(kind * env.cellest_n) + c];
    if (v != 0.) unsafeAtomicAdd(&global_array[(int64_t)c * env.est_stride], v);
  }
}
// One workgroup of 768 threads per CU: 3 waves/SIMD at 168 VGPRs (the LDS tables allow two workgroups per CU, so 256-thread
// workgroups stop at 2 waves/SIMD whatever their registers). Measured against 256 x 2 (2 waves/SIMD, 256 VGPRs): k_rpkt
// 352 -> 339 ms (classic), 398 -> 379 (kilonova_lte), k_rpkt + k_bfest_dense 825 -> 781 (nltenebular); 1024 x 1 (4
// waves/SIMD, 128 VGPRs, 768 B of scratch): 457 ms.
#ifndef ARTIS_RPKT_TB
#define ARTIS_RPKT_TB 768  // threads per workgroup of k_rpkt ...
#define ARTIS_RPKT_WGS 1   // ... and workgroups per CU
#endif
// LINE_LDS (ARTIS_AMD_LINELDS=1; instead of the continuum table, which it leaves no room for): the line list's frequencies
// (globals::linelist nu, rpkt.cc:106-207 get_possible_event: one of the two reads per line visited, the other being the cell's
// population factor) in LDS, the whole list when it has at most LINE_LDS_MAX lines. What a per-cell, per-wave WINDOW of
// {frequency, population factor} pairs would need -- many lanes of a wave in one cell and one stretch of the list -- the
// cell-sorted work list does not give: a wave's 64 packets sit in ~21 cells (2.6 lanes per cell) and
// anywhere in the spectrum. Measured slower than the continuum table in LDS: profiles/r04/line_window.md.
constexpr int LINE_LDS_MAX = 14336;  // lines (112 KB)
template <bool CONT_LDS, int TB, bool LINE_LDS = false>
__global__ void __launch_bounds__(TB, ARTIS_RPKT_WGS) k_rpkt(Env env, const int32_t *list, int32_t n, Lists next,
                                                                   unsigned long long *gstats, int budget, int32_t *cursors, int nchunks,
                                                                   int drain_budget) {
  __shared__ stat_t lstats[ARTIS_NSTATS];
  __shared__ ContPack lds_cont[CONT_LDS ? CONT_LDS_MAX : 1];
  __shared__ double lds_line_nu[LINE_LDS ? LINE_LDS_MAX : 1];
  __shared__ double lds_cellest[3 * ((CONT_LDS || LINE_LDS) ? RPKT_CELLEST_CAP : RPKT_CELLEST_CAP_NOCONT)];
  constexpr int NEC = LINE_LDS ? 1 : ESTCACHE_SLOTS;       // (the line list in LDS leaves no room for the caches)
  __shared__ double lds_estcache[(TB / 64) * NEC * 3];   // per wave: the accumulators of ESTCACHE_SLOTS cells (physics.h Env::estcache) ...
  __shared__ int32_t lds_esttag[(TB / 64) * NEC * 2];    // ... whose cells they are, and the claims of an eviction
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  cellest_begin(env, lds_cellest, env.cellest_n_r, TB, env.E.J, env.E.nuJ, env.E.ffheatingestimator);
  env.estcache = nullptr;
  env.estcache_nv = 0;
  if (!LINE_LDS && env.estcache_on && env.cellest_n_r == 0) {  // many cells: the wave's own cache instead of the workgroup's array
    const int w = threadIdx.x >> 6;
    env.estcache_nv = 3;
    env.estcache = lds_estcache + (w * NEC * 3);
    env.estcache_tag = lds_esttag + (w * NEC * 2);
    for (int l = threadIdx.x & 63; l < NEC; l += 64) {
      env.estcache_tag[l] = -1;
      env.estcache_tag[NEC + l] = -1;
      env.estcache[(l * 3) + 0] = 0.;
      env.estcache[(l * 3) + 1] = 0.;
      env.estcache[(l * 3) + 2] = 0.;
    }
  }
  if (LINE_LDS) {
    for (int i = threadIdx.x; i < env.M.nlines; i += TB) lds_line_nu[i] = env.M.line_nu[i];
    env.M.line_nu = lds_line_nu;
  }
  if (CONT_LDS) {
    const D2 *src = (const D2 *)env.M.cont_pack;
    D2 *dst = (D2 *)lds_cont;
    for (int i = threadIdx.x; i < env.M.nbfcontinua * 2; i += TB) dst[i] = src[i];
    env.M.cont_pack = lds_cont;
    env.cont_in_lds = 1;
  }
  __syncthreads();
  env.stats = lstats;
  const double ts_end = env.S.ts_end;
  Puller q;
  puller_init(q, n, nchunks);
  bool have = false;
  bool drained = false;  // the launch's work list is used up (k_thermal: same hand-over to the next launch)
  int32_t pi = 0;
  int steps = 0;
  Pkt p;
  Chi x;
#ifdef ARTIS_PROFILE
  long long tprev = clock64();
#endif
  while (true) {
    const int32_t idx = pull(q, !have, cursors);
    if (idx >= 0) {
      pi = list[idx];
      pkt_load(env.P, pi, p);
      chi_load(env.P, pi, p, x);
      steps = 0;
      have = true;
    }
    if (!drained && q.exhausted) {
      drained = true;
      if ((threadIdx.x & 63) == 0) __hip_atomic_store(&cursors[MAX_CHUNKS], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!drained && drain_budget < budget && (steps & 1) == 0)
      drained = __hip_atomic_load(&cursors[MAX_CHUNKS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    if (!__any(have)) {
      if (q.exhausted) break;
      continue;
    }
#define ROUND_LEAVE(n) ((n) >= budget || (drained && (n) >= drain_budget))
#define ROUND_PUT(kind_, pi_) append_by_kind(kind_, pi_, p.cellindex, p.nu_cmf, next, (p.ma_element * 5 + p.ma_ion))
#include "rpkt_round.inc"
#undef ROUND_LEAVE
#undef ROUND_PUT
  }
  __syncthreads();
  if (env.estcache != nullptr) {  // the wave's accumulators go to the cells' records: a lane per slot
    for (int l = threadIdx.x & 63; l < NEC; l += 64) {
      const int cell = env.estcache_tag[l];
      if (cell < 0) continue;
      const double s0 = env.estcache[(l * 3) + 0], s1 = env.estcache[(l * 3) + 1], s2 = env.estcache[(l * 3) + 2];
      if (s0 != 0.) unsafeAtomicAdd(&env.E.J[(int64_t)cell * env.est_stride], s0);
      if (s1 != 0.) unsafeAtomicAdd(&env.E.nuJ[(int64_t)cell * env.est_stride], s1);
      if (s2 != 0.) unsafeAtomicAdd(&env.E.ffheatingestimator[(int64_t)cell * env.est_stride], s2);
    }
  }
  cellest_flush(env, CELLEST_J, env.E.J, TB);
  cellest_flush(env, CELLEST_NUJ, env.E.nuJ, TB);
  cellest_flush(env, CELLEST_FFHEAT, env.E.ffheatingestimator, TB);
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}

#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
// The deferred updates of the detailed bound-free estimators (radfield.cc:215). A record's continua are the kept ones of
// its window [begin, end); LPR lanes share the record (cell, frequency, weight) and take one kept continuum each, so the
// lanes are busy however long the window is (a lane-per-packet loop ran at 17 % of the lanes). Which continuum is the
// k-th kept one of the window comes from two small per-cell tables made with the keep bitmap (k_keptlist): the kept
// continua as a list, and the number of kept continua below each bitmap word -- two reads and two bit counts give the
// window's places [r0, r1) in the list. (Before: prefix sums of the words' bit counts over the lanes, a bisection with six
// ds_bpermute and a select-k-th-bit per lane and round: 2.5x the VALU instructions.) The contributions are the ones
// update_bfestimators() would have added in place (same arithmetic); only the order of the f64 atomic additions differs.
// (Keeping a cell's sums in LDS across a run of records of the same cell -- per wave, or per workgroup with ds_add_f64 --
// was measured and lost, 651 / 427 ms against 364 ms; so did sorting the records by cell first and summing a cell's whole
// run in an LDS row, 1101 vs 989 ms for k_rpkt + this kernel, profiles/r03/bfest_sorted_lds_rows.patch. Compiled out, the
// additions are worth 98 of the 989 ms.)
// CONT_LDS: the static continuum table (ContPack, two of a contribution's ~six 16-byte reads) is staged in LDS by a
// workgroup of DENSE_TB threads, one per CU.
constexpr int DENSE_TB = 1024;
// LPR lanes per record: a window holds ~30 kept continua (ARTIS_AMD_DENSE_LPR = 64, 32 or 16)
#ifndef ARTIS_DENSE_WGS
#define ARTIS_DENSE_WGS 2  // workgroups of DENSE_TB threads per CU: 8 waves/SIMD at 60 VGPRs (1: 4 waves/SIMD; k_rpkt + this kernel 781 -> 774 ms)
#endif
template <bool CONT_LDS, int TB, int LPR>
__global__ void __launch_bounds__(TB, (TB == DENSE_TB ? ARTIS_DENSE_WGS : 1)) k_bfest_dense(Env env) {
  __shared__ ContPack lds_cont[CONT_LDS ? CONT_LDS_MAX : 1];
  if (CONT_LDS) {
    const D2 *src = (const D2 *)env.M.cont_pack;
    D2 *dst = (D2 *)lds_cont;
    for (int i = threadIdx.x; i < env.M.nbfcontinua * 2; i += TB) dst[i] = src[i];
    env.M.cont_pack = lds_cont;
    env.cont_in_lds = 1;
    __syncthreads();
  }
  static_assert(LPR == 64 || LPR == 32 || LPR == 16, "lanes per record");
  const DevModel &M = env.M;
  const int n = min(*env.bfev_count, env.bfev_cap);
  const int lane = threadIdx.x & (LPR - 1);
  const int unit = (blockIdx.x * TB + threadIdx.x) / LPR;
  const int nunits = gridDim.x * (TB / LPR);
  for (int ei = unit; ei < n; ei += nunits) {
    const BfEvent ev = env.bfev[ei];
    const int c = ev.c;
    const double nu = ev.nu;
    const float T_e = env.C.Te[c];
    // the record's continua are the kept ones of [begin, end): places [r0, r1) of the cell's list of kept continua
    int r0, r1;
    kept_range(env, c, ev.begin, ev.end, r0, r1);
    const double ex = exp(-HOVERKB * nu / T_e);
    const bool split_usable = (ex >= DBLMIN);
    const int32_t *list = env.K.allcont_keptlist + (krow(env, c) * M.nbfcontinua);
    const D2 *keptpair = env.K.allcont_keptpair + (krow(env, c) * M.nbfcontinua);
    // the sums go to the continuum's place in the list when the call keeps them there (all cells resident), else to its
    // estimator: ~30 additions of a record then fall into 4-5 neighbouring 64-byte sectors instead of ~16 scattered ones
    // (k_rpkt + this kernel 978 -> 858 ms per step; with the additions compiled out: 891)
    double *dst = env.bfrate_kept ? env.bfrate_kept + ((int64_t)c * M.nbfcontinua) : env.E.bfrate_raw + ((int64_t)c * M.nbfestim);
    for (int r = r0 + lane; r < r1; r += LPR) {
      const int i = list[r];
      const double ep = keptpair[r].y;
      const int bi = bfestimindex(M, i);
      if (bi >= 0) ARTIS_EST_ADD(&dst[env.bfrate_kept ? r : bi], bf_sigma_contr_ep(env, c, i, nu, T_e, ex, split_usable, ep) * ev.w);
    }
  }
}
// the sums kept by place in the list go to their estimators (one wave per cell; the places are left zero for the next call)
__global__ void __launch_bounds__(BLOCK) k_bfrate_expand(Env env) {
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const DevModel &M = env.M;
  if (wave >= M.npts_nonempty) return;
  const int c = (int)wave;
  const int nw = M.nkeepwords;
  const int nkept = env.K.allcont_keepprefix[(krow(env, c) * nw) + nw - 1] + __popcll(env.K.allcont_keepbits[(krow(env, c) * nw) + nw - 1]);
  const int32_t *list = env.K.allcont_keptlist + (krow(env, c) * M.nbfcontinua);
  double *kept = env.bfrate_kept + ((int64_t)c * M.nbfcontinua);
  double *dst = env.E.bfrate_raw + ((int64_t)c * M.nbfestim);
  for (int r = lane; r < nkept; r += 64) {
    const double v = kept[r];
    if (v != 0.) {
      dst[bfestimindex(M, list[r])] += v;  // (a continuum without an estimator was never added to: v == 0)
      kept[r] = 0.;
    }
  }
}
#endif
