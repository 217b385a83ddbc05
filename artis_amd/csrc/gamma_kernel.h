// gamma_kernel.h -- k_gamma: gamma packets and the deposits they end in, one do_gamma() call per iteration (physics.h). Included by artis_engine.hip inside its anonymous namespace.
#pragma once
// gamma packets (and the non-thermal deposits they end in): one do_gamma() call per iteration, same persistent
// work-pulling form as k_rpkt; a packet that has thermalised leaves as a k-packet for the thermal list
#ifndef ARTIS_GAMMA_WAVES
#define ARTIS_GAMMA_WAVES 2
#endif
__global__ void __launch_bounds__(BLOCK, ARTIS_GAMMA_WAVES) k_gamma(Env env, const int32_t *list, int32_t n, Lists next,
                                                                     unsigned long long *gstats, int budget, int32_t *cursors, int nchunks) {
  __shared__ stat_t lstats[ARTIS_NSTATS];
  __shared__ double lds_cellest[GAMMA_CELLEST_CAP];
  __shared__ double lds_scalars[ARTIS_NSCALARS];
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  scalars_begin(env, lds_scalars);
  cellest_begin(env, lds_cellest, env.cellest_n_g, BLOCK, env.E.dep_estimator_gamma);
  __syncthreads();
  env.stats = lstats;
  const double ts_end = env.S.ts_end;
  Puller q;
  puller_init(q, n, nchunks);
  bool have = false;
  int32_t pi = 0;
  int steps = 0;
  Pkt p;
  while (true) {
    const int32_t idx = pull(q, !have, cursors);
    if (idx >= 0) {
      pi = list[idx];
      pkt_load(env.P, pi, p);
      steps = 0;
      have = true;
    }
    if (!__any(have)) {
      if (q.exhausted) break;
      continue;
    }
    int kind = NEXT_DONE;
    int32_t out_pi = 0;
    if (have) {
      bool go = gamma_can_continue(p, ts_end);
      if (go) {
        go = gamma_iter(env, p, pi);
        steps++;
      }
      if (!go || steps >= budget) {
        pkt_store(env.P, pi, p);
        kind = classify(env, p, ts_end);
        out_pi = pi;
        have = false;
      }
    }
    append_by_kind(kind, out_pi, p.cellindex, p.nu_cmf, next, (p.ma_element * 5 + p.ma_ion));
  }
  __syncthreads();
  cellest_flush(env, CELLEST_DEPGAMMA, env.E.dep_estimator_gamma, BLOCK);
  scalars_flush(env);
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}
