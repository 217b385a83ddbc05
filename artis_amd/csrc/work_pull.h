// work_pull.h -- how the persistent, work-pulling kernels hand the indices of their work list to their waves (rpkt_kernels.h "the propagation
// kernels"): Puller, puller_init(), chunk_at(), pull(). Included by rpkt_kernels.h inside artis_engine.hip's namespace; the same text compiles for the host under
// ARTIS_HOST_EMU (tests/pull_host), where one host thread stands for a wave: it calls puller_place() and pull_wave() with the mask of its asking
// lanes. No includes of its own: <cstdint> comes from the including file.
//
// The list is cut into `nchunks` contiguous chunks with one cursor each; a wave takes from its home chunk, then from its own XCD's chunks, then from
// the rest (chunk_at). Every index of [0, n) is handed out exactly once. Placement only: never a result.
#pragma once
#ifdef ARTIS_HOST_EMU
#define PULL_FN inline
#define PULL_FETCH_ADD(p, v) __atomic_fetch_add((p), (v), __ATOMIC_RELAXED)
#define PULL_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define PULL_POPC(m) __builtin_popcountll(m)
#else
#define PULL_FN __device__ inline
#define PULL_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PULL_POPC(m) __popcll(m)
#endif
constexpr int MAX_CHUNKS = 8192;  // >= 256 CUs x 4 waves/SIMD x 4 SIMDs, a multiple of 8
// cursors[]: [0, MAX_CHUNKS) the chunk cursors | [MAX_CHUNKS] the launch's "list used up" flag
constexpr int PULL_SLOTS = MAX_CHUNKS + 1;

struct Puller {
  int chunk;           // current chunk
  int32_t cbeg, cend;  // ... and its range of the list (kept: the bounds cost two 64-bit divisions)
  int home, cx;        // first position of the search order: (XCD, local index); chunks per XCD
  int nchunks;
  bool exhausted;
  int32_t n;           // the list's length
};
PULL_FN int64_t chunk_begin(int32_t n, int c, int nchunks) { return ((int64_t)n * c) / nchunks; }
// A wave at (XCD, index within the XCD) and a list of n entries in nchunks chunks (a multiple of 8)
PULL_FN void puller_place(Puller &q, int xcd, int local, int32_t n, int nchunks) {
  q.nchunks = nchunks;
  q.cx = nchunks >> 3;
  q.home = xcd * q.cx + (local % q.cx);
  q.n = n;
  q.chunk = q.home;
  q.cbeg = (int32_t)chunk_begin(n, q.chunk, nchunks);
  q.cend = (int32_t)chunk_begin(n, q.chunk + 1, nchunks);
  q.exhausted = false;
}
#ifndef ARTIS_HOST_EMU
// chunk_mode: 0 = one chunk per wave (or fewer, shared in order), 1 = per workgroup, 2 = per COMPUTE UNIT (nchunks == 256):
// the workgroups that the hardware placed on one CU walk one run of cells together, so the CU's L1 sees a handful of
// cells. The CU is read from HW_REG_HW_ID (MI355X: 8 XCDs x 4 shader engines x 8 CUs, CU_ID 0..7 or 1..8).
__device__ inline void puller_init(Puller &q, int32_t n, int nchunks, int chunk_mode = 0) {
  int xcd = blockIdx.x & 7;
  // wave / workgroup / CU index within its XCD
  int local = (chunk_mode == 1) ? (int)(blockIdx.x >> 3) : (int)(blockIdx.x >> 3) * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
  if (chunk_mode == 2) {
    unsigned hwid, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcd = (int)(xcc & 7u);
    local = (int)(((hwid >> 13) & 3u) * 8u + ((hwid >> 8) & 7u));
  }
  puller_place(q, xcd, local, n, nchunks);
}
#endif
// position v of a wave's search order -> chunk: its own XCD's chunks first (from its home chunk, wrapping), then the rest
PULL_FN int chunk_at(const Puller &q, int v) {
  const int x0 = (q.home / q.cx) * q.cx;
  if (v < q.cx) return x0 + ((q.home - x0 + v) % q.cx);
  return (x0 + v) % q.nchunks;
}
// does chunk c still have entries? A cursor only grows, so a stale read can only make a chunk look fuller than it is: the
// next pull finds out.
PULL_FN bool chunk_has(const Puller &q, int c, int32_t *cursors) {
  const int32_t used = PULL_LOAD(&cursors[c]);
  return chunk_begin(q.n, c, q.nchunks) + used < chunk_begin(q.n, c + 1, q.nchunks);
}
// The wave's two collective steps. mask: the asking lanes (not empty).
#ifdef ARTIS_HOST_EMU
PULL_FN int wave_fetch_add(int32_t *p, int v, unsigned long long) { return PULL_FETCH_ADD(p, v); }
// the first chunk of the search order (after the current one) that has entries becomes the current one; false: none has
PULL_FN bool wave_next_chunk(Puller &q, int32_t *cursors) {
  for (int v = 1; v < q.nchunks; v++) {
    const int c = chunk_at(q, v);
    if (chunk_has(q, c, cursors)) {
      q.chunk = c;
      q.cbeg = (int32_t)chunk_begin(q.n, c, q.nchunks);
      q.cend = (int32_t)chunk_begin(q.n, c + 1, q.nchunks);
      return true;
    }
  }
  return false;
}
#else
__device__ inline int wave_fetch_add(int32_t *p, int v, unsigned long long mask) {
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(p, v);
  return __shfl(base, leader);
}
// ... 64 candidates at a time (the unserved lanes ask again)
__device__ inline bool wave_next_chunk(Puller &q, int32_t *cursors) {
  const int lane = threadIdx.x & 63;
  for (int v0 = 1; v0 < q.nchunks; v0 += 64) {
    const int v = v0 + lane;
    bool has = false;
    int c = 0;
    if (v < q.nchunks) {
      c = chunk_at(q, v);
      has = chunk_has(q, c, cursors);
    }
    const unsigned long long hm = __ballot(has);
    if (hm != 0) {
      q.chunk = __shfl(c, __ffsll((long long)hm) - 1);
      q.cbeg = (int32_t)chunk_begin(q.n, q.chunk, q.nchunks);
      q.cend = (int32_t)chunk_begin(q.n, q.chunk + 1, q.nchunks);
      return true;
    }
  }
  return false;
}
#endif
// One pull of a wave whose lanes in `mask` ask (wave-uniform; q.exhausted is false): the p-th asking lane takes list index *first + p if that is
// below *end, else nothing this time.
PULL_FN void pull_wave(Puller &q, unsigned long long mask, int32_t *cursors, int64_t *first, int64_t *end) {
  const int cnt = PULL_POPC(mask);
  const int64_t cbeg = q.cbeg, cend = q.cend;
  const int base = wave_fetch_add(&cursors[q.chunk], cnt, mask);
  *first = cbeg + base;
  *end = cend;
  // this chunk is used up: look for one that still has entries
  if (cbeg + base + cnt > cend && !wave_next_chunk(q, cursors)) q.exhausted = true;
}
#ifndef ARTIS_HOST_EMU
// Hands list indices to the lanes with need==true. Returns the index for this lane or -1. Wave-uniform control flow.
__device__ inline int32_t pull(Puller &q, bool need, int32_t *cursors) {
  need = need && !q.exhausted;
  const unsigned long long mask = __ballot(need);
  if (mask == 0) return -1;
  const int lane = threadIdx.x & 63;
  const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
  int64_t first, end;
  pull_wave(q, mask, cursors, &first, &end);
  const int64_t mine = first + prefix;
  return (need && mine < end) ? (int32_t)mine : -1;
}
#endif
