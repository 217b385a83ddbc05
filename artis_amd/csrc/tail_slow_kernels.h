// tail_slow_kernels.h -- k_tail (the last few thousand packets, one per lane through every kind of step), k_slow (the deferred bound-free actions, PEND_*) and
// k_blackbody. Included by artis_engine.hip inside its anonymous namespace.
#pragma once
// Tail kernel: the LAST few thousand r-packets and thermal packets of a timestep, one per lane, each carried through
// r-packet steps, macro-atom walks and k-packet steps until it leaves these kinds (end of the timestep, escape, a
// slow-path action, a gamma-ray type, a blackbody step, another cache tile). The event-split kernels need one launch
// pair per r-packet <-> thermal alternation of the longest-lived packets, and a launch lasts as long as its slowest
// packet: with the nltenebular options 530 of 720 launches of a step hold fewer than 10^4 packets and cost 490 ms
// (the last 150 hold 1-5 packets). Here the packets do not wait for each other. Same functions in the same order per
// packet as the split kernels (state goes through the packet record at every change of kind, as it does between
// launches), so the same results; a fat kernel (both bodies: scratch, low occupancy), which is why it is the tail only.
struct TailLists {
  const int32_t *list[4];  // the current r-packet, thermal, slow-path and blackbody lists
  int32_t n[4];
};
#ifndef ARTIS_TAIL_WAVES
#define ARTIS_TAIL_WAVES 2
#endif
#ifndef ARTIS_SLOW_WAVE_FB
#define ARTIS_SLOW_WAVE_FB 1  // free-bound emission frequencies selected by the wave (physics.h FbSel) in k_slow and k_tail
#endif
#ifndef ARTIS_TAIL_WAVE_CHI
#define ARTIS_TAIL_WAVE_CHI 1  // k_tail: the continuum opacity of a step evaluated by the wave (physics.h chi_rpkt_cont_wave); 0: by the packet's lane
#endif
#ifndef ARTIS_SLOW_WAVE_FB_MAX
#define ARTIS_SLOW_WAVE_FB_MAX 6  // ... in k_slow for waves with at most this many emissions
#endif
// (Round 5: with the static tables of a transition's target in LDS as in k_thermal -- workgroups of 8 packets, one per compute unit -- the
// classic tail took 27.6 / 26.7 ms against 29.0 / 25.3, the nltenebular tail 123 against 108: profiles/r05/tail_profile.txt. Not kept.)
__global__ void __launch_bounds__(BLOCK, ARTIS_TAIL_WAVES) k_tail(Env env, TailLists in, Lists next, unsigned long long *gstats) {
  __shared__ stat_t lstats[ARTIS_NSTATS];
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  __syncthreads();
  env.stats = lstats;
  env.ma_concurrent_fill = 1;  // this kernel's waves fill pool records while others read them: published places are read with acquire (physics.h ma_rowtab_acquire)
  const double ts_end = env.S.ts_end;
  // ONE PACKET PER WAVE (lane 0): packets in different kinds of step would otherwise serialise inside a wave (measured
  // with a packet per lane: slower than the split kernels); the tail has fewer packets than the GPU has waves
  const int64_t tid = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  int kind = NEXT_DONE;
  int32_t pi = 0, cellindex = 0;
  double nu_cmf = 0.;
  // (every lane runs the loop over the packet's kinds of step with lane 0's kind; only lane 0 holds the packet and carries the steps out,
  // the other 63 join it where the wave works together: the frequency of a free-bound emission, physics.h FbSel)
  const bool owner = (threadIdx.x & 63) == 0 && tid < (int64_t)in.n[0] + in.n[1] + in.n[2] + in.n[3];
  Pkt p;
  if (owner) {
    int32_t j = (int32_t)tid;
    int which = 0;
    while (j >= in.n[which]) j -= in.n[which++];
    pi = in.list[which][j];
    pkt_load(env.P, pi, p);
  }
#ifdef ARTIS_PROFILE_TAIL
  // (-DARTIS_PROFILE_TAIL, tools/tail_profile.py) clocks / 16 of the owner lane by kind of step: slots 42 slow, 43 r-packet, 44 thermal, 45 blackbody,
  // 46 / 47 the r-packet and thermal iterations; 50..53 the same clocks of the waves that ran longer than 2^25 clocks (~15 ms) only
  long long tp[4] = {0, 0, 0, 0};
  long long tp_n[2] = {0, 0};
#define TAILP(i, code)                   \
  {                                      \
    const long long tp0_ = clock64();    \
    code;                                \
    tp[i] += clock64() - tp0_;           \
  }
#else
#define TAILP(i, code) code
#endif
  while (true) {
    if (owner) kind = classify(env, p, ts_end);
    const int kind_w = __builtin_amdgcn_readfirstlane(__shfl(kind, 0));
    if (kind_w == NEXT_SLOW) {
      if (env.ion_absent != nullptr) {
        // the packet waits for a static record the population left out (tables.h "ABSENT IONS"): it leaves for the slow-path list, whose kernel
        // fills such records -- between launches, where no wave reads a record while another writes it (the host runs that list next)
        const bool hand = owner && ma_waits_for_static_fill(env, p);
        if (__builtin_amdgcn_readfirstlane(__shfl((int)hand, 0)) != 0) break;  // (kind is NEXT_SLOW)
      }
#ifdef ARTIS_PROFILE_TAIL
      const long long tps0 = clock64();
#endif
#if ARTIS_SLOW_WAVE_FB
      FbSel sel;
      sel.mode = 1;
      sel.valid = false;
      sel.element = sel.lowerion = sel.lower = sel.t = 0;
      sel.T_e = 0.f;
      sel.zrand = sel.nu = 0.;
      if (owner && slow_selects_continuum_nu(p)) {
        Pkt t = p;
        (void)advance_slow(env, t, pi, &sel);
      }
      fbsel_wave(env, sel);
#endif
      {
        int fc = 0, ful = 0;
        int32_t funit = 0;
        const bool fill = ARTIS_MA_WAVE_FILL && owner && p.pend == PEND_MA_FILL && ma_slow_fill_claim(env, p, &fc, &ful, &funit);
        ma_fill_wave(env, fill, fc, ful);
        if (fill) ma_slow_fill_publish(env, fc, ful, funit);
      }
#if ARTIS_SLOW_WAVE_FB
      if (owner) (void)advance_slow(env, p, pi, sel.valid ? &sel : nullptr);
#else
      if (owner) (void)advance_slow(env, p, pi);
#endif
      {
        // the pool of on-demand records is used up and the packet still waits for a record: it leaves for the slow-path list (the host empties
        // the pool before that list's next launch); nothing in this kernel could end the wait
        // (only a packet whose level has no record and none being filled: one whose record another wave is filling goes on -- ADVICE r05)
        const bool waits = owner && env.M.ncold > 0 && p.pend != PEND_NONE &&
                           __hip_atomic_load(env.ma_pool_full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 && ma_record_absent(env, p);
        if (__builtin_amdgcn_readfirstlane(__shfl((int)waits, 0)) != 0) {
          if (owner) kind = NEXT_SLOW;
          break;
        }
      }
#ifdef ARTIS_PROFILE_TAIL
      tp[0] += clock64() - tps0;
#endif
    } else if (kind_w == NEXT_RPKT) {
      // every lane runs the loop over the packet's steps; before a step that evaluates the continuum opacity (do_rpkt_step()'s own conditions:
      // rpkt_step_evaluates_chi) the WAVE evaluates it -- the window's kept continua side by side, their terms added by the packet's lane in
      // the sequential loop's order (physics.h chi_bf_gammacontr_wave) -- and the step finds it in the packet's cache
      Chi x;
      if (owner) chi_load(env.P, pi, p, x);
      bool go = owner && rpkt_can_continue(p, ts_end);
#ifdef ARTIS_PROFILE_TAIL
      const long long tpr0 = clock64();
#endif
      while (__builtin_amdgcn_readfirstlane(__shfl((int)go, 0)) != 0) {
#if ARTIS_TAIL_WAVE_CHI
        int cc = 0;
        const bool need = go && rpkt_step_evaluates_chi(env, p, x, &cc);
        if (__builtin_amdgcn_readfirstlane(__shfl((int)need, 0)) != 0) {
          const int cw = __builtin_amdgcn_readfirstlane(__shfl(cc, 0));
          const double nuw = wave_bcast(p.nu_cmf, 0);
          const int piw = __builtin_amdgcn_readfirstlane(__shfl(pi, 0));
          chi_rpkt_cont_wave(env, nuw, x, cw, (int64_t)piw, owner);
        }
#endif
        if (go) {
          go = rpkt_iter(env, p, pi, x);
#ifdef ARTIS_PROFILE_TAIL
          tp_n[0]++;
#endif
        }
      }
#ifdef ARTIS_PROFILE_TAIL
      tp[1] += clock64() - tpr0;
#endif
      if (owner) chi_store(env.P, pi, p, x);
    } else if (kind_w == NEXT_MA || kind_w == NEXT_KPKT) {
      if (owner) {
        MACtx k = ma_ctx(env, p);
        bool go = thermal_can_continue(p, ts_end);
#ifdef ARTIS_PROFILE_TAIL
        const long long tpt0 = clock64();
        while (go) {
          (void)thermal_iter(env, p, pi, k, &go);
          tp_n[1]++;
        }
        tp[2] += clock64() - tpt0;
#else
        while (go) (void)thermal_iter(env, p, pi, k, &go);
#endif
      }
    } else if (kind_w == NEXT_BB) {
      TAILP(3, if (owner) (void)advance_blackbody(env, p, pi));
    } else {
      break;
    }
  }
#ifdef ARTIS_PROFILE_TAIL
  if (owner) {
    const bool longwave = (tp[0] + tp[1] + tp[2] + tp[3]) > (1LL << 25);
    for (int i = 0; i < 4; i++) {
      atomicAdd(&lstats[42 + i], (stat_t)(tp[i] >> 4));
      if (longwave) atomicAdd(&lstats[50 + i], (stat_t)(tp[i] >> 4));
    }
    atomicAdd(&lstats[46], (stat_t)tp_n[0]);
    atomicAdd(&lstats[47], (stat_t)tp_n[1]);
    if (longwave) {
      atomicAdd(&lstats[54], (stat_t)1);
      atomicAdd(&lstats[55], (stat_t)tp_n[0]);
      atomicAdd(&lstats[56], (stat_t)tp_n[1]);
    }
  }
#endif
  if (owner) {
    pkt_store(env.P, pi, p);
    cellindex = p.cellindex;
    nu_cmf = p.nu_cmf;
  }
  append_by_kind(kind, pi, cellindex, nu_cmf, next);
  __syncthreads();
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}

// slow path: the rare bound-free actions (rate coefficients with exp(), adaptive Gauss-Kronrod frequency sampling)
// (round 6, with the build's machine LICM off: the classic options' slow path fits 167 VGPRs with 2 spilled, i.e. 3 waves per SIMD instead of 2;
// the builds with interpolated cross-sections / the nebular family need 170-256 and keep what the compiler chooses)
#ifndef ARTIS_SLOW_EU
// (the nebular family's -- NLTE populations, the non-thermal channels -- takes 256 VGPRs + 22 AGPRs alone at one wave per SIMD; held to 256 it
// spills 48 and runs two: k_slow 70.6 -> 51.4 ms, nltenebular step 1018 -> 1001 ms (profiles/r06/ab_slow.txt); kilonova_lte: no difference)
#define ARTIS_SLOW_EU (ARTIS_OPT_PHIXS_CLASSIC_NO_INTERPOLATION ? 3 : (ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? 2 : 1))
#endif
__global__ void __launch_bounds__(BLOCK, ARTIS_SLOW_EU) k_slow(Env env, const int32_t *list, int32_t n, Lists next, unsigned long long *gstats) {
  __shared__ stat_t lstats[ARTIS_NSTATS];
  __shared__ double lds_scalars[ARTIS_NSCALARS];
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  scalars_begin(env, lds_scalars);
  __syncthreads();
  env.stats = lstats;
  env.ma_concurrent_fill = 1;  // this kernel's waves fill pool records while others read them: published places are read with acquire (physics.h ma_rowtab_acquire)
  const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int kind = NEXT_DONE;
  int32_t pi = 0, cellindex = 0;
  double nu_cmf = 0.;
  // A free-bound emission's frequency (select_continuum_nu ratecoeff.cc:563: up to a hundred adaptive 31-point quadratures) is selected by
  // the WAVE (physics.h FbSel): the action is first run on a copy of the packet up to the selection, whose arguments are recorded; the
  // wave's lanes evaluate the abscissae of each rule side by side for one recorded selection after the other; then the action runs for real.
  // (Round 4: one lane per emission while the other lanes of its wave waited -- lane utilisation 0.11; ARTIS_SLOW_WAVE_FB=0 builds that form.)
  const bool mine = tid < n;
  Pkt p;
  FbSel sel;
  sel.mode = 1;
  sel.valid = false;
  sel.element = sel.lowerion = sel.lower = sel.t = 0;
  sel.T_e = 0.f;
  sel.zrand = sel.nu = 0.;
  if (mine) {
    pi = list[tid];
    pkt_load(env.P, pi, p);
#ifdef ARTIS_PROFILE_SLOW
    atomicAdd(&lstats[48 + (p.pend < 9 ? p.pend : 9)], (stat_t)1);  // (-DARTIS_PROFILE_SLOW: the slow-path visits by kind of pending action, stats slots 48..57)
#endif
  }
#if ARTIS_SLOW_WAVE_FB
  {
    // (only where a few lanes of the wave have an emission: the wave takes them one after the other, each ~9x faster than a lane; with many --
    // the nltenebular family, where a bound-free action is pending in nearly every round -- the lanes' own selections side by side are faster:
    // k_slow 83 ms with the wave's form throughout against 68 ms)
    const bool isfb = mine && slow_selects_continuum_nu(p);
    const int nfb = __popcll(__ballot(isfb));
    if (nfb > 0 && nfb <= ARTIS_SLOW_WAVE_FB_MAX) {
      if (isfb) {
        Pkt t = p;
        (void)advance_slow(env, t, pi, &sel);
      }
      fbsel_wave(env, sel);
    }
  }
#endif
  if (env.ion_absent != nullptr) {  // a static record the population left out (tables.h "ABSENT IONS"): claimed by the lane, filled by the wave
    int sc = 0, sul = 0;
    // (... or that an action of the packet's macro-atom needs again after a refill of its row: physics.h ma_waits_for_static_fill)
    const bool sfill = mine && ma_waits_for_static_fill(env, p) && ma_static_fill_claim(env, p, &sc, &sul);
    ma_fill_wave<true>(env, sfill, sc, sul);
  }
  {  // a cold level's record (PEND_MA_FILL): claimed by the lane, filled by the wave, published by the lane
    int fc = 0, ful = 0;
    int32_t funit = 0;
    const bool fill = ARTIS_MA_WAVE_FILL && mine && p.pend == PEND_MA_FILL && ma_slow_fill_claim(env, p, &fc, &ful, &funit);
    ma_fill_wave(env, fill, fc, ful);
    if (fill) ma_slow_fill_publish(env, fc, ful, funit);
  }
  if (mine) {
    kind = advance_slow(env, p, pi, sel.valid ? &sel : nullptr);
    pkt_store(env.P, pi, p);
    cellindex = p.cellindex;
    nu_cmf = p.nu_cmf;
  }
  append_by_kind(kind, pi, cellindex, nu_cmf, next);
  __syncthreads();
  scalars_flush(env);
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}

// blackbody emission of pre-k-packets and of k-packets in grey cells: one do_kpkt_blackbody() per packet
__global__ void __launch_bounds__(BLOCK) k_blackbody(Env env, const int32_t *list, int32_t n, Lists next, unsigned long long *gstats) {
  __shared__ stat_t lstats[ARTIS_NSTATS];
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  __syncthreads();
  env.stats = lstats;
  const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int kind = NEXT_DONE;
  int32_t pi = 0, cellindex = 0;
  double nu_cmf = 0.;
  if (tid < n) {
    pi = list[tid];
    Pkt p;
    pkt_load_thermal(env.P, pi, p);
    kind = advance_blackbody(env, p, pi);
    pkt_store_thermal(env.P, pi, p);
    cellindex = p.cellindex;
    nu_cmf = p.nu_cmf;
  }
  append_by_kind(kind, pi, cellindex, nu_cmf, next);
  __syncthreads();
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}
