// late_kernel.h -- k_late: the end of a population -- r-packets, thermal packets and slow-path actions -- in one persistent launch, waves taking roles over
// per-workgroup rings (LateArgs, LateRing, LateSink). Included by artis_engine.hip inside its anonymous namespace.
#pragma once
// ---- k_late: the END of a population -- the r-packets and thermal packets left once the lists are too short to fill the GPU -- in ONE persistent
// launch. The split kernels put a device-wide barrier between every r-packet <-> thermal alternation, and below ~1e6 packets every such round costs a
// floor (its slowest packet's visit) however few packets it holds; the sum over rounds of those maxima is far above the longest single chain. Here a
// packet goes from one kind of step to the other inside the launch:
//   geometry   one workgroup of LATE_TB = 512 threads per compute unit (2 waves per SIMD, no spilled register; 768 threads: 3 waves, 34 spilled, measured);
//   ownership  workgroup b owns a fixed contiguous share of the (sorted) r-packet list and of the thermal list; a packet never changes workgroup, and
//              nothing waits on another workgroup;
//   queues     per workgroup one ring per role (r-packet, thermal, slow path) in its slice of a scratch array, capacity = the workgroup's share (a packet sits in
//              at most one queue); head, reserved and published tail in LDS. A producer stores the packet (the bodies' pkt_store / chi_store /
//              pkt_store_thermal), writes the entries it reserved, and publishes them in reservation order with a workgroup-scope release; a consumer
//              reads the published tail with a workgroup-scope acquire, reads the entries, and takes them with a compare-and-swap on the head (entries
//              [head, published) cannot be overwritten while the head stands: the ring holds as many entries as the workgroup has packets). All waves
//              of a workgroup share a compute unit and its L1: no device-scope fence;
//   roles      a wave runs one role at a time (all its lanes in the same body: rpkt_round.inc / thermal_round.inc, the split kernels' own); idle lanes pull
//              from the role's queue; a lane keeps its packet until its kind changes or it ends -- no budget. The waves start split between the roles
//              in proportion to the workgroup's two shares (at least one wave each where both are non-empty); a wave whose lanes are all idle and whose
//              queue is empty takes the other role if that queue is not empty;
//   slow path  the third role: the rare bound-free actions (k_slow's body: the wave selects the free-bound frequencies of its lanes' emissions, then
//              advance_slow()), one pull - action - store - put per pass, nothing held between passes. The last wave of a workgroup serves only this
//              queue (ARTIS_LATE_SLOW_WAVE; it polls with s_sleep while the workgroup has packets), and every other wave whose lanes are all idle looks
//              at the slow queue first: a packet with a pending action waits for a poll, not for the launch to end and two more to begin;
//   ejection   a packet whose next kind is a blackbody step, a gamma-ray kind, or that is done, is stored and appended to the ordinary
//              lists (append_by_kind) exactly as a split kernel would; the host's loop runs those kinds and what comes back is listed again;
//   the end    `live` (LDS) counts the workgroup's packets that have not been ejected; a wave leaves when it is 0;
//   estimators plain f64 global atomics (the lists are short here): no per-wave caches, no few-cells LDS arrays;
//   waits      every wait is for a wave of the same workgroup, so progress is certain; each is capped all the same. An idle wave polls with s_sleep at
//              most poll_cap times, then counts itself in *bailouts and leaves (it holds no packet; the waves that do carry the workgroup's packets to
//              their end: a bail-out costs time, never an answer). A producer waits for the reservations before its own to be published -- a few
//              instructions of another wave -- and, if that never happens, raises error flag 47 and publishes nothing (the call fails; no entry is read that was not written).
// Dynamic LDS: [stats | counters | LevelPack x nlevels | uint16 target levels x nalltrans | ContPack x nbfcontinua] (late_lds_bytes()).
#ifndef ARTIS_LATE_KERNEL
#define ARTIS_LATE_KERNEL (!ARTIS_OPT_VPKT_ON && !ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON)  // the builds that may use k_late
#endif
#ifndef ARTIS_LATE_TB
#define ARTIS_LATE_TB 512  // 2 waves per SIMD at up to 256 VGPRs: no spilled register (768: 3 waves at 168 VGPRs, 34 spilled; profiles/r08/late_kernel.md)
#endif
#ifndef ARTIS_LATE_SLOW_INLINE
// the slow role's body inside k_late's loop, or called from it. Classic options: 255 VGPRs and no spilled register inlined, 26 spilled around the call.
// The builds with interpolated cross-sections, whose slow path alone takes 256 VGPRs + 22 AGPRs (k_slow): 398 spilled inlined, 95 called
// (profiles/r10/late_slow_role.md)
#define ARTIS_LATE_SLOW_INLINE ARTIS_OPT_PHIXS_CLASSIC_NO_INTERPOLATION
#endif
#ifndef ARTIS_LATE_SLOW_WAVE
#define ARTIS_LATE_SLOW_WAVE 1  // the last wave of each workgroup serves the slow-path queue only; 0: idle waves alone do (profiles/r10/late_slow_role.md)
#endif
constexpr int LATE_TB = ARTIS_LATE_TB;
constexpr size_t LATE_LDS_HEAD = (sizeof(stat_t) * ARTIS_NSTATS) + 64;  // statistics, then the queues' counters
inline size_t late_lds_bytes(int nlevels, int nalltrans, int nbfcontinua) {
  return LATE_LDS_HEAD + (sizeof(LevelPack) * (size_t)nlevels) + (((sizeof(uint32_t) * (size_t)((nalltrans + 1) / 2)) + 15) & ~(size_t)15) +
         (sizeof(ContPack) * (size_t)nbfcontinua);
}
constexpr int LATE_NQ = 3;  // roles and their queues: 0 = r-packets, 1 = thermal packets, 2 = the slow path
struct LateArgs {
  const int32_t *list[LATE_NQ];  // the r-packet, the thermal and the slow-path list, consumed whole
  int32_t n[LATE_NQ];
  int32_t *ring[LATE_NQ];        // scratch: [n[0] + n[1] + n[2]] each; workgroup b's slice begins at the sum of its three shares' beginnings
  int32_t *bailouts;
  int32_t poll_cap;
#ifdef ARTIS_PROFILE_LATE
  int32_t *stamp;  // [packets] when a packet entered the slow queue (clocks / 16, low word)
#endif
};
#if ARTIS_LATE_KERNEL
struct LateRing {
  int32_t *ring;   // the workgroup's slice
  uint32_t cap;
  int32_t *head, *res, *pub;  // LDS: entries taken | reserved by producers | published (head <= pub <= res <= head + cap)
};
__device__ inline void late_push(const LateRing &Q, bool flag, int32_t pi, int32_t *errflag) {
  const unsigned long long mask = __ballot(flag);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63;
  const int cnt = __popcll(mask);
  const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(Q.res, cnt);
  base = __shfl(base, leader);
  if (flag) Q.ring[(uint32_t)(base + prefix) % Q.cap] = pi;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the packet records and the entries, before the entries are published
  if (lane == leader) {
    int spins = 0;
    bool turn = true;
    while (__hip_atomic_load(Q.pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != base) {  // earlier reservations are published first
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 24)) {
        // never publish over a reservation that was not: the entries stay out of reach, the workgroup's waves run into their poll caps, the
        // kernel ends and the call fails with this flag
        if (errflag) *errflag = 47;
        turn = false;
        break;
      }
    }
    if (turn) __hip_atomic_store(Q.pub, base + cnt, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}
// hands queue entries to the lanes with need == true: the packet's index, or -1. Wave-uniform control flow.
__device__ inline int32_t late_pull(const LateRing &Q, bool need) {
  const unsigned long long mask = __ballot(need);
  if (mask == 0) return -1;
  const int lane = threadIdx.x & 63;
  const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
  const int leader = __ffsll((long long)mask) - 1;
  int h = 0, t = 0;
  if (lane == leader) {
    h = __hip_atomic_load(Q.head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    t = __hip_atomic_load(Q.pub, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  h = __shfl(h, leader);
  t = __shfl(t, leader);
  const int take = min(__popcll(mask), t - h);
  if (take <= 0) return -1;
  int32_t v = -1;
  if (need && prefix < take) v = __hip_atomic_load(&Q.ring[(uint32_t)(h + prefix) % Q.cap], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  int ok = 0;
  if (lane == leader) ok = (atomicCAS(Q.head, h, h + take) == h) ? 1 : 0;  // another wave took them first: the caller asks again
  ok = __shfl(ok, leader);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  // the packet records are read after this
  return ok ? v : -1;
}
// k_late's policy for the loop bodies it shares with the split kernels (rpkt_round.inc, thermal_round.inc): no budget; a packet that stays an
// r-packet or a thermal packet, or has a slow-path action pending, goes to the workgroup's queue of that role, every other packet leaves the kernel
struct LateSink {
  LateRing q[LATE_NQ];
  int32_t *live;
  int32_t *errflag;
#ifdef ARTIS_PROFILE_LATE
  int32_t *stamp;
#endif
  // left: this lane gave up packet pi, whose next kind is `kind`. Wave-uniform control flow.
  // to_list: a slow-path packet that leaves the kernel for the ordinary slow-path list (it waits for a record k_slow has to fill)
  __device__ void put(bool left, int kind, int32_t pi, const Pkt &p, const Lists &next, bool to_list = false) const {
    const bool to_r = left && kind == NEXT_RPKT;
    const bool to_t = left && (kind == NEXT_MA || kind == NEXT_KPKT);
    // (a packet that waits for a static record the population left out -- tables.h "ABSENT IONS"; this kernel runs where no level is cold --
    // leaves for the ordinary slow-path list like the kinds the kernel cannot run: k_slow fills such records, between launches)
    // (from the r-packet and thermal roles that is PEND_MA_FILL alone: an action's record was populated when it was drawn from a moment ago; the
    // slow role passes to_list for every packet physics.h ma_waits_for_static_fill() flags)
    const bool to_s = left && kind == NEXT_SLOW && p.pend != PEND_MA_FILL && !to_list;
#ifdef ARTIS_PROFILE_LATE
    if (to_s) stamp[pi] = (int32_t)(clock64() >> 4);
#endif
    late_push(q[0], to_r, pi, errflag);
    late_push(q[1], to_t, pi, errflag);
    late_push(q[2], to_s, pi, errflag);
    const bool out = left && !to_r && !to_t && !to_s;
    append_by_kind(out ? kind : NEXT_DONE, pi, p.cellindex, p.nu_cmf, next, (p.ma_element * 5 + p.ma_ion));
    const unsigned long long om = __ballot(out);
    if (om != 0 && (int)(threadIdx.x & 63) == __ffsll((long long)om) - 1) atomicSub(live, __popcll(om));  // after the append: `live` 0 = all is on the lists
  }
};
// One pass of the slow-path role: k_slow's body for the packets the wave's lanes have just pulled (got >= 0), without the cold-record fill (no cold
// levels where k_late runs). The wave selects the free-bound frequencies whatever their number, as in k_tail. Wave-uniform control flow.
#if ARTIS_LATE_SLOW_INLINE
__device__ inline
#else
__device__ __noinline__
#endif
void late_slow_round(const Env &env, const LateSink &sink, const Lists &next, int32_t got) {
  const bool mine = got >= 0;
  const int32_t pi = mine ? got : 0;
  Pkt p;
  p.cellindex = 0; p.nu_cmf = 0.; p.ma_element = 0; p.ma_ion = 0;
  FbSel sel;
  sel.mode = 1;
  sel.valid = false;
  sel.element = sel.lowerion = sel.lower = sel.t = 0;
  sel.T_e = 0.f;
  sel.zrand = sel.nu = 0.;
  if (mine) pkt_load(env.P, pi, p);
#ifdef ARTIS_PROFILE_LATE
  // (-DARTIS_PROFILE_LATE) stats slots: 42 clocks / 16 the packets waited in the slow queue, 43 the packets, 44 / 45 those that waited longer than
  // 2^12 / 2^16 units (31 us / 0.5 ms at 2.1 GHz), 46 passes of the role, 47 clocks / 16 of the passes (per wave)
  const long long tpass0 = clock64();
  if (mine) {
    const uint32_t w = (uint32_t)((int32_t)(tpass0 >> 4) - sink.stamp[pi]);
    atomicAdd(&env.stats[42], (stat_t)w);
    atomicAdd(&env.stats[43], (stat_t)1);
    if (w > (1u << 12)) atomicAdd(&env.stats[44], (stat_t)1);
    if (w > (1u << 16)) atomicAdd(&env.stats[45], (stat_t)1);
  }
#endif
  if (mine && slow_selects_continuum_nu(p)) {
    Pkt t = p;
    (void)advance_slow(env, t, pi, &sel);
  }
  fbsel_wave(env, sel);
  int kind = NEXT_DONE;
  const bool waits = mine && ma_waits_for_static_fill(env, p);
  if (waits) {
    kind = NEXT_SLOW;  // (put() sends it on to k_slow, untouched)
  } else if (mine) {
    kind = advance_slow(env, p, pi, sel.valid ? &sel : nullptr);
    pkt_store(env.P, pi, p);
  }
  sink.put(mine, kind, pi, p, next, waits);
#ifdef ARTIS_PROFILE_LATE
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&env.stats[46], (stat_t)1);
    atomicAdd(&env.stats[47], (stat_t)((clock64() - tpass0) >> 4));
  }
#endif
}
__global__ void __launch_bounds__(LATE_TB, 1) k_late(Env env, LateArgs a, Lists next, unsigned long long *gstats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char late_lds[];
  // this workgroup's shares of the three lists (contiguous; neighbouring shares on one XCD: xcd_chunk) and its slice of the rings
  const int64_t nwg = gridDim.x, b = xcd_chunk(blockIdx.x, nwg);
  const int32_t r0 = (int32_t)(((int64_t)a.n[0] * b) / nwg), r1 = (int32_t)(((int64_t)a.n[0] * (b + 1)) / nwg);
  const int32_t t0 = (int32_t)(((int64_t)a.n[1] * b) / nwg), t1 = (int32_t)(((int64_t)a.n[1] * (b + 1)) / nwg);
  const int32_t s0 = (int32_t)(((int64_t)a.n[2] * b) / nwg), s1 = (int32_t)(((int64_t)a.n[2] * (b + 1)) / nwg);
  const int32_t own = (r1 - r0) + (t1 - t0) + (s1 - s0);
  if (own == 0) return;  // (the whole workgroup)
  stat_t *lstats = (stat_t *)late_lds;
  int32_t *ctr = (int32_t *)(late_lds + (sizeof(stat_t) * ARTIS_NSTATS));  // head r, t | reserved r, t | published r, t | live | head, reserved, published s
  LevelPack *lds_levelpack = (LevelPack *)(late_lds + LATE_LDS_HEAD);
  uint16_t *lds_tlevel = (uint16_t *)(lds_levelpack + env.M.nlevels);
  ContPack *lds_cont = (ContPack *)((unsigned char *)lds_tlevel + (((sizeof(uint32_t) * (size_t)((env.M.nalltrans + 1) / 2)) + 15) & ~(size_t)15));
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  for (int i = threadIdx.x; i < env.M.nlevels; i += LATE_TB) lds_levelpack[i] = env.M.level_pack[i];
  {
    const uint32_t *src = (const uint32_t *)env.M.alltrans_tlevel16;  // (the allocation is padded to whole words)
    uint32_t *dst = (uint32_t *)lds_tlevel;
    for (int i = threadIdx.x; i < (env.M.nalltrans + 1) / 2; i += LATE_TB) dst[i] = src[i];
  }
  {
    const D2 *src = (const D2 *)env.M.cont_pack;
    D2 *dst = (D2 *)lds_cont;
    for (int i = threadIdx.x; i < env.M.nbfcontinua * 2; i += LATE_TB) dst[i] = src[i];
  }
  const int32_t slice = r0 + t0 + s0;
  LateSink sink{{{a.ring[0] + slice, (uint32_t)own, ctr + 0, ctr + 2, ctr + 4}, {a.ring[1] + slice, (uint32_t)own, ctr + 1, ctr + 3, ctr + 5},
                 {a.ring[2] + slice, (uint32_t)own, ctr + 7, ctr + 8, ctr + 9}},
                ctr + 6, env.errflag
#ifdef ARTIS_PROFILE_LATE
                , a.stamp
#endif
  };
  // the queues begin with the workgroup's shares
  for (int i = threadIdx.x; i < r1 - r0; i += LATE_TB) sink.q[0].ring[i] = a.list[0][r0 + i];
  for (int i = threadIdx.x; i < t1 - t0; i += LATE_TB) sink.q[1].ring[i] = a.list[1][t0 + i];
  for (int i = threadIdx.x; i < s1 - s0; i += LATE_TB) {
    sink.q[2].ring[i] = a.list[2][s0 + i];
#ifdef ARTIS_PROFILE_LATE
    a.stamp[a.list[2][s0 + i]] = (int32_t)(clock64() >> 4);
#endif
  }
  if (threadIdx.x == 0) {
    ctr[0] = ctr[1] = ctr[7] = 0;
    ctr[2] = ctr[4] = r1 - r0;
    ctr[3] = ctr[5] = t1 - t0;
    ctr[8] = ctr[9] = s1 - s0;
    ctr[6] = own;
  }
  env.M.level_pack = lds_levelpack;
  env.M.alltrans_tlevel16 = lds_tlevel;
  env.ma_tables_in_lds = 1;
  env.M.cont_pack = lds_cont;
  env.cont_in_lds = 1;
  env.cellest_lds = nullptr;
  env.cellest_n = 0;
  env.estcache = nullptr;
  env.estcache_nv = 0;
  __syncthreads();
  env.stats = lstats;
  const double ts_end = env.S.ts_end;
  constexpr int NW = LATE_TB / 64;
  constexpr int NW_RT = ARTIS_LATE_SLOW_WAVE ? NW - 1 : NW;  // the waves that begin in the r-packet and thermal roles
  // roles: 0 = r-packets, 1 = thermal packets, 2 = the slow path (`home`: the role of the first two a wave came from)
  const int32_t own_rt = (r1 - r0) + (t1 - t0);
  int nw_r = own_rt > 0 ? (int)((((int64_t)(r1 - r0) * NW_RT) + (own_rt / 2)) / own_rt) : 0;
  if (r1 > r0 && t1 > t0) nw_r = max(1, min(NW_RT - 1, nw_r));
  const bool slow_wave = ARTIS_LATE_SLOW_WAVE && __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == NW - 1;
  int home = __builtin_amdgcn_readfirstlane(((int)(threadIdx.x >> 6) < nw_r) ? 0 : 1);
  int role = slow_wave ? 2 : home;
  const auto waiting = [&](int q) {  // entries published and not yet taken
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(sink.q[q].pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) -
                                          __hip_atomic_load(sink.q[q].head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
  };
  bool have = false;
  int32_t pi = 0;
  int n_it = 0;  // (the bodies count the lane's steps / units; no budget reads them here)
  int polls = 0;
  Pkt p;
  Chi x;
  MACtx k;
  long long tprev = 0;
  while (true) {
    const int32_t got = late_pull(sink.q[role], !have);
    if (role == 2) {  // (no lane of a wave in this role holds a packet between passes)
      if (__any(got >= 0)) {
        late_slow_round(env, sink, next, got);
        polls = 0;
        continue;
      }
    } else if (got >= 0) {
      pi = got;
      if (role == 0) {
        pkt_load(env.P, pi, p);
        chi_load(env.P, pi, p, x);
      } else {
        pkt_load_thermal(env.P, pi, p);  // the hot line only
        k = ma_ctx(env, p);
      }
      have = true;
    }
    if (!__any(have)) {
      // a wave whose lanes are all idle: the slow queue first (a packet there waits for nothing else), then its own role's, then the other's
      if (waiting(2) > 0) {
        role = 2;
        continue;
      }
      if (!slow_wave) {
        role = home;
        if (waiting(home) > 0) continue;  // (another wave was faster: ask again)
        if (waiting(1 - home) > 0) {
          role = home = 1 - home;
          continue;
        }
      }
      if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(ctr + 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0) break;
      if (++polls > a.poll_cap) {  // the other waves hold what is left and carry it to its end
        if ((threadIdx.x & 63) == 0) atomicAdd(a.bailouts, 1);
        break;
      }
      __builtin_amdgcn_s_sleep(64);
      continue;
    }
    polls = 0;
    const bool held = have;
    constexpr bool COLD = false;  // (no cold levels where this kernel runs)
#define ROUND_LEAVE(n) false
#define ROUND_BEFORE_LEAVE
#define ROUND_PUT(kind_, pi_) sink.put(held && !have, kind_, pi_, p, next)
    if (role == 0) {
      int &steps = n_it;
#include "rpkt_round.inc"
    } else {
      int &units = n_it;
#include "thermal_round.inc"
    }
#undef ROUND_LEAVE
#undef ROUND_BEFORE_LEAVE
#undef ROUND_PUT
  }
  __syncthreads();
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}
#endif
