// thermal_kernels.h -- k_thermal: k-packets and walking macro-atoms in one persistent kernel, its body thermal_round.inc. Included by artis_engine.hip inside its anonymous namespace.
#pragma once
// Thermal packets (k-packets and walking macro-atoms) are advanced by ONE persistent kernel, so that the k-packet ->
// macro-atom -> k-packet cycle (tens of times per packet and timestep, kpkt.cc:51) needs no kernel boundary.
//
// Staging macro-atom records in LDS was built and measured in rounds 2 and 3 (per-workgroup slots holding the hot levels'
// records of the cells in flight, k_thermal<true>; and k_thermal_q, walk contexts in per-wave LDS slots with lanes refilled
// inside the transition loop): both bit-identical, both slower (profiles/r02/lds_staging.md,
// profiles/r03/k_thermal_lane_compaction.md). Round 4 took the cumulative sums and targets those variants staged out of
// the records altogether (tables.h), and the variants with them.
#ifndef ARTIS_THERMAL_WAVES
#define ARTIS_THERMAL_WAVES 4
#endif
// Fused thermal kernel, phase form (physics.h thermal_iter): up to ARTIS_MA_PHASE macro-atom transitions, then one
// k-packet step, per iteration; lanes take a new packet between iterations. Workgroups of TB threads on the XCD chunks.
#ifndef ARTIS_THERMAL_TB
#define ARTIS_THERMAL_TB BLOCK                 // threads per workgroup of k_thermal,
#define ARTIS_THERMAL_EU ARTIS_THERMAL_WAVES   // the waves per SIMD its registers are to allow (512 / EU VGPRs) ...
#define ARTIS_THERMAL_WGS ARTIS_THERMAL_WAVES  // ... and its workgroups per CU
#endif
// 1: k_thermal holds no rate-coefficient code: a search its filters cannot decide (3e-4 per transition) is handed to the slow-path
// kernel with the draw in the packet's pend fields (physics.h PEND_MA_SEARCH / _RADSEARCH / PEND_KPKT_COLLEXC), which re-adds the sums
// and carries on; the packet is back on the thermal list for the next launch. With the code inlined here the kernel spilled 122
// instead of 21 registers, reloaded around every phase: 200 GB of scratch traffic per step.
// (Not in the builds with detailed bound-free estimators -- the nltenebular family: their steps are made of twice as many launch rounds,
// and every hand-over costs a packet the rest of its launch: measured 1417 ms with, 1403 without.)
#ifndef ARTIS_THERMAL_SPLIT_EXACT
#define ARTIS_THERMAL_SPLIT_EXACT (ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? 0 : 1)
#endif
#ifndef ARTIS_MA_DEFER_EXACT
#define ARTIS_MA_DEFER_EXACT 1  // the re-adding of a search's sums outside the transition loop (physics.h ma_jump_internal<true>)
#endif
// TABLES_LDS: the two static tables a transition's target is read from -- the target level of every entry of alltrans
// (2 bytes) and the LevelPack of every level (16 bytes) -- are copied into LDS once per workgroup (one workgroup of 1024
// threads per CU: the same 4 waves/SIMD at 128 VGPRs), and a transition reads its target with two ds_reads instead of a
// 16-byte gather from the static target table in L2: of a transition's three dependent reads (action filter; the
// direction's filter, in the sector the first one brought; the target) one long wait is left. For atomic data whose
// tables fit (MA_LDS_LEVELS / MA_LDS_TRANS: the bench's 1567 levels and 27 238 entries take 80 KB); larger data keep the
// target table in HBM. Static tables, the same for every cell: nothing to stage per cell (what lost in rounds 2-3).
// TABLES_LDS = 2: atomic data whose alltrans table does not fit (the 110 860-line set: 221 720 entries) keep the 2-byte target
// levels in HBM (443 KB instead of the 3.5 MB of 16-byte targets: L2-resident beside the cells' records) and the LevelPack
// table alone in LDS (up to MA_LDS_LEVELS2 levels).
constexpr int MA_LDS_LEVELS = 2048;   // 32 KB
constexpr int MA_LDS_TRANS = 32768;   // 64 KB
constexpr int MA_LDS_LEVELS2 = 9856;  // 154 KB (round 6: 6144 = 96 KB until the workgroup's per-cell estimator accumulators -- 32 KB that only models
                                      // with few cells use -- were left out of this form: the 4e5-line set's 8 457 levels fit now; a model with few cells AND
                                      // more than MA_LDS_LEVELS levels takes the form without LDS tables)
template <int TB, int TABLES_LDS, bool COLD = false>
__global__ void __launch_bounds__(TB, (TABLES_LDS ? 1 : ARTIS_THERMAL_EU)) k_thermal(Env env, const int32_t *list, int32_t n, Lists next,
                                                                     unsigned long long *gstats, int budget, int32_t *cursors,
                                                                     int nchunks, int chunk_mode, int drain_budget) {
  __shared__ stat_t lstats[ARTIS_NSTATS];
  __shared__ double lds_cellest[TABLES_LDS == 2 ? 1 : THERMAL_CELLEST_CAP];
  __shared__ LevelPack lds_levelpack[TABLES_LDS == 1 ? MA_LDS_LEVELS : (TABLES_LDS == 2 ? MA_LDS_LEVELS2 : 1)];
  __shared__ uint16_t lds_tlevel[TABLES_LDS == 1 ? MA_LDS_TRANS : 8];
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  cellest_begin(env, lds_cellest, env.cellest_n_t, TB, env.E.colheatingestimator);
  env.estcache = nullptr;
  env.estcache_nv = 0;
  // many cells: the workgroup's array is not in use; its LDS holds the waves' caches of per-cell sums instead (physics.h Env::estcache): per wave
  // ESTCACHE_SLOTS doubles, then per wave 2 x ESTCACHE_SLOTS int32 (the slots' cells, the claims)
  static_assert(TABLES_LDS == 2 || (TB / 64) * ESTCACHE_SLOTS * 2 <= THERMAL_CELLEST_CAP, "the waves' estimator caches take the few-cells array's LDS");
  if (TABLES_LDS != 2 && env.estcache_on && env.cellest_n_t == 0) {
    const int w = threadIdx.x >> 6;
    env.estcache = lds_cellest + (w * ESTCACHE_SLOTS);
    env.estcache_tag = (int32_t *)(lds_cellest + ((TB / 64) * ESTCACHE_SLOTS)) + (w * ESTCACHE_SLOTS * 2);
    env.estcache_nv = 1;
    for (int l = threadIdx.x & 63; l < ESTCACHE_SLOTS; l += 64) {
      env.estcache[l] = 0.;
      env.estcache_tag[l] = -1;
      env.estcache_tag[ESTCACHE_SLOTS + l] = -1;
    }
  }
  if (TABLES_LDS) {
    for (int i = threadIdx.x; i < env.M.nlevels; i += TB) lds_levelpack[i] = env.M.level_pack[i];
    env.M.level_pack = lds_levelpack;
    if (TABLES_LDS == 1) {
      const uint32_t *src = (const uint32_t *)env.M.alltrans_tlevel16;  // (the allocation is padded to whole words)
      uint32_t *dst = (uint32_t *)lds_tlevel;
      for (int i = threadIdx.x; i < (env.M.nalltrans + 1) / 2; i += TB) dst[i] = src[i];
      env.M.alltrans_tlevel16 = lds_tlevel;
    }
    env.ma_tables_in_lds = 1;
  }
  __syncthreads();
  env.stats = lstats;
  const double ts_end = env.S.ts_end;
  Puller q;
  puller_init(q, n, nchunks, chunk_mode);
  bool have = false;
  int32_t pi = 0;
  int units = 0;
  bool drained = false;  // the launch's work list is used up (any wave found out)
  Pkt p;
  MACtx k;
#ifdef ARTIS_PROFILE
#define PROF_ADD(slot, dt) \
  do {                     \
    if ((threadIdx.x & 63) == 0) atomicAdd(&lstats[slot], (stat_t)((dt) >> 4)); \
  } while (0)
  long long tprev = clock64();
#endif
  while (true) {
    const int32_t idx = pull(q, !have, cursors);
    if (idx >= 0) {
      pi = list[idx];
      pkt_load_thermal(env.P, pi, p);  // the hot line only
      k = ma_ctx(env, p);
      units = 0;
      have = true;
    }
    if (!__any(have)) {
      if (q.exhausted) break;
      continue;
    }
    // Once the work list is used up, the launch lasts as long as its slowest packets keep their lanes (up to `budget`
    // units each) while the rest of the GPU idles. In a launch whose successor is large anyway (drain_budget set by the
    // host), a packet then leaves after drain_budget units for that next launch, where its work runs beside a full list.
    // (Where a packet is handed from launch to launch never changes it: budgets are placement, tested.)
    // BEFORE the list is used up such a launch has no unit budget (the host passes budget = INT_MAX, launch_thermal(); ARTIS_AMD_BUDGET_T_BULK
    // gives it one): holding the lane costs nothing while the wave's other lanes keep pulling, and the hand-over ends the launch anyway. A budget
    // there only stored, listed, sorted and loaded a long history again every round, and left it to run alone at the step's end.
#define ROUND_BEFORE_LEAVE \
    if (!drained && q.exhausted) { \
      drained = true; \
      if ((threadIdx.x & 63) == 0) __hip_atomic_store(&cursors[MAX_CHUNKS], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
    } \
    if (!drained && drain_budget < budget) \
      drained = __hip_atomic_load(&cursors[MAX_CHUNKS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
#define ROUND_LEAVE(n) ((n) >= budget || (drained && (n) >= drain_budget))
#define ROUND_PUT(kind_, pi_) append_by_kind(kind_, pi_, p.cellindex, p.nu_cmf, next, (p.ma_element * 5 + p.ma_ion))
#include "thermal_round.inc"
#undef ROUND_BEFORE_LEAVE
#undef ROUND_LEAVE
#undef ROUND_PUT
  }
  __syncthreads();
  if (env.estcache_nv == 1) {  // the wave's sums go to the cells' records
    for (int l = threadIdx.x & 63; l < ESTCACHE_SLOTS; l += 64) {
      const int cell = env.estcache_tag[l];
      const double s0 = env.estcache[l];
      if (cell >= 0 && s0 != 0.) unsafeAtomicAdd(&env.E.colheatingestimator[(int64_t)cell * env.est_stride], s0);
    }
  }
  cellest_flush(env, CELLEST_COLHEAT, env.E.colheatingestimator, TB);
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}
