// vpkt_kernel.h -- k_vpkt: the virtual packets of the events the launch before recorded, one lane per (event, observer direction) (physics.h trace_vpkts). Empty unless
// the options preset has VPKT_ON. Included by artis_engine.hip inside its anonymous namespace.
#pragma once
#if ARTIS_OPT_VPKT_ON
// Virtual packets (vpkt.cc): the emissions and electron scatterings the launch before recorded (physics.h trace_vpkts), one
// lane per (event, observer direction): the optical depths of every opacity choice along the ray to the grid's edge, then
// the attenuated energy into that observer's spectrum (f64 atomics). Nothing of the real packets is read or written.
// Persistent and work-pulling like the propagation kernels: a lane whose ray has ended (left the grid, absorbed beyond tau_max, met a
// thick cell) takes the next (event, observer) pair at once -- rays cross 1 ... 50 cells, and with one ray per lane from start to end a
// wave lasted as long as its longest.
#ifndef ARTIS_VPKT_WGS
#define ARTIS_VPKT_WGS 4
#endif
#ifndef ARTIS_VPKT_TB
#define ARTIS_VPKT_TB 768  // threads of the one workgroup per CU of the form with the continuum table in LDS: 3 waves/SIMD at 168 VGPRs.
                          // Virtual-packet bench (1e6 packets, t = 5 d): 1470 / 1284 / 1290 ms per step at 1024 / 768 / 512 (MI355X, round 4)
#endif
constexpr int VPKT_CHUNKS = 2048;
// CONT_LDS (round 4): the static continuum table in LDS as in k_rpkt -- every cell a ray crosses sums the bound-free opacity
// (chi_bf_gammacontr) -- with ONE workgroup of 1024 threads per CU instead of four of 256 (the same 4 waves/SIMD).
template <bool CONT_LDS, int TB>
__global__ void __launch_bounds__(TB, (CONT_LDS ? 1 : ARTIS_VPKT_WGS)) k_vpkt(Env env, unsigned long long *gstats, int32_t *cursors) {
  __shared__ stat_t lstats[ARTIS_NSTATS];
  __shared__ ContPack lds_cont[CONT_LDS ? CONT_LDS_MAX : 1];
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  if (CONT_LDS) {
    const D2 *src = (const D2 *)env.M.cont_pack;
    D2 *dst = (D2 *)lds_cont;
    for (int i = threadIdx.x; i < env.M.nbfcontinua * 2; i += TB) dst[i] = src[i];
    env.M.cont_pack = lds_cont;
    env.cont_in_lds = 1;
  }
  __syncthreads();
  env.stats = lstats;
  const int nobs = env.M.vpkt->nobsdirections;
  const int64_t n64 = (int64_t)min(*env.vpkt_count, env.vpkt_cap) * nobs;
  const VpktSeed *queue = env.vpkt_queue;
  if (n64 < 0x7FFFFFF0LL) {
    const int32_t n = (int32_t)n64;
    Puller q;
    puller_init(q, n, VPKT_CHUNKS);
    bool have = false;
    VRay ray;
    while (true) {
      const int32_t idx = pull(q, !have, cursors);
      if (idx >= 0) have = vray_begin_seed(env, queue[idx / nobs], idx % nobs, ray);
      if (!__any(have)) {
        if (q.exhausted) break;
        continue;
      }
      if (have) have = vray_step(env, ray);
    }
  } else {  // (more pairs than a list index holds: one ray per lane from start to end)
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n64; i += (int64_t)gridDim.x * TB) {
      const VpktSeed seed = queue[i / nobs];
      vpkt_trace_seed_direction(env, seed, (int)(i % nobs));
    }
  }
  __syncthreads();
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}
#endif
