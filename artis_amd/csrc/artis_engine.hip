// artis_engine.hip -- the MI355X packet-propagation engine behind include/artis_amd.h.
//
// Layout of the work on the GPU (gfx950, wave64):
//   * model tables, cell state and the per-cell cache live in HBM for the whole timestep;
//   * packets are three arrays of cache-line records (tables.h PktStore: hot / flight / cold), one lane per packet;
//   * one timestep = populate kernels (cell cache) + repeated k_propagate launches over a compacted
//     list of packets that still need updating. Each thread advances its packet by at most `budget`
//     do_packet() calls, then survivors are appended to the next list with a wave ballot;
//   * estimators are accumulated with hardware f64 atomics, event counters in LDS and flushed per block.
// There is no CPU path in this library: every entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is bound at run time (rccl_api below)

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <cmath>

#include "model_build.h"
#include "engine_config.h"
#include "cache_residency.h"
#include "physics.h"
#include "radfield_fit.h"
#include "ion_balance.h"
#include "decay_update.h"
#include "deposition.h"
#include "packet_init.h"
#include "thermal_balance.h"
#include "bf_heating.h"
#include "ratecoeff_tables.h"
#include "photoion.h"
#include "spectra.h"

#include <rocprim/device/device_radix_sort.hpp>

using namespace artis;

namespace {

thread_local std::string g_last_error;

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);                            \
      return ARTIS_ERR_HIP;                                                                        \
    }                                                                                              \
  } while (0)

constexpr int BLOCK = 256;

#include "cellcache_kernels.h"  // ------------------------------------------------ populate kernels

// ------------------------------------------------------------------ packet layout kernels
// The slot of a packet is not its index in the caller's array: slots are handed out in the order of the packets'
// propagation cells at upload (perm[slot] = index in the caller's array), so that the lanes of a wave -- whose work list
// is sorted by cell -- read and write neighbouring records. Thermal packets never leave their cell, r-packets drift away
// from this order only gradually. perm == nullptr: identity.
__global__ void __launch_bounds__(BLOCK) k_aos_to_rec(const artis_packet *aos, PktStore P, const int32_t *perm) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < P.n) aos_to_rec(aos[perm ? perm[i] : i], P, i);
}
__global__ void __launch_bounds__(BLOCK) k_rec_to_aos(PktStore P, artis_packet *aos, const int32_t *perm) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < P.n) rec_to_aos(P, i, aos[perm ? perm[i] : i]);
}
__global__ void __launch_bounds__(BLOCK) k_aos_cellkeys(const artis_packet *aos, int64_t n, int32_t ngrid, int32_t *ident, int32_t *keys) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  ident[i] = (int32_t)i;
  const int32_t c = aos[i].cellindex;
  keys[i] = (c >= 0 && c < ngrid) ? c : 0;  // a packet of a type this path does not own may carry any cell index
}

// append (pi, key) of every lane with flag set to list[] / keys[], one atomic per wave (wave-ballot compaction)
// (the sort counts the keys itself, in LDS, a tile of the list at a time: k_sort_tilehist)
__device__ inline void wave_append(bool flag, int32_t pi, int32_t key, int32_t *list, int32_t *keys, int32_t *count) {
  const unsigned long long mask = __ballot(flag);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63;
  const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
  int base = 0;
  const int leader = __ffsll((long long)mask) - 1;
  if (lane == leader) base = atomicAdd(count, __popcll(mask));
  base = __shfl(base, leader);
  if (flag) {
    list[base + prefix] = pi;
    keys[base + prefix] = key;
  }
}

// Blocks are dealt round-robin over the 8 XCDs (each with its own L2). The work lists are sorted by cell, so give
// every XCD one contiguous eighth of the list: the per-cell tables its waves read then stay in that XCD's L2.
// (Bijective remap of blockIdx -> list chunk; placement only changes speed, never results.)
__device__ inline int64_t xcd_chunk(int64_t b, int64_t nb) {
  const int64_t q = nb / 8, r = nb % 8, xcd = b % 8;
  return ((xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + b / 8;
}

// Work lists, one per kind of pending work (physics.h NEXT_*). A kernel consumes the whole current list of ITS kind and
// appends packets to the current lists of the other kinds; packets that stay with the kernel's own kind (launch budget
// used up) go to that kind's alternate list, which becomes its current list afterwards. Every entry carries its sort
// key (physics.h list_sort_key), written by the lane that still has the packet in registers, so that sorting a list
// never touches the packet records.
struct Lists {
  int32_t *lst[NEXT_NKINDS];  // current list of each kind
  int32_t *key[NEXT_NKINDS];  // ... and the sort keys of its entries
  int32_t *counts;            // [NEXT_NKINDS] fill counts of the current lists
  int32_t self_kind;          // kind of the running kernel
  int32_t *self_list;         // its alternate list
  int32_t *self_key;
  int32_t *self_count;
  int32_t kpkt_slot;          // list that takes k-packets: NEXT_KPKT, or NEXT_MA when k-packets and macro-atoms share the
                              // fused thermal kernel
  int32_t nubins;             // frequency bins of the r-packet list's keys (1 = sort by cell only)
  int32_t mabins;             // sub-keys of the thermal list's keys (1 = sort by cell only)
  int32_t numajor;            // > 0 = the cell groups of the grid: r-packet keys with the frequency bin as the MAJOR part (ARTIS_AMD_SORT_NUMAJOR=0: cell-major)
  int32_t cellshift;          // ... groups of 2^cellshift cells with neighbouring indices share a key (ARTIS_AMD_SORT_CELLSHIFT)
};
// ma_sub: (tuning, ARTIS_AMD_MABINS=16) a sub-key 0..15 of a thermal-list entry below its cell, -1: none
__device__ inline void append_by_kind(int kind, int32_t pi, int32_t cellindex, double nu_cmf, const Lists &L, int ma_sub = -1) {
  const int slot = (kind == NEXT_KPKT) ? L.kpkt_slot : kind;
  int32_t key = list_sort_key(cellindex, nu_cmf, (slot == NEXT_RPKT) ? L.nubins : 1);
  if (slot == NEXT_RPKT && L.numajor > 0 && L.nubins > 1) key = ((key % SORT_NUBINS) * L.numajor) + ((key / SORT_NUBINS) >> L.cellshift);
  if (slot == NEXT_MA && L.mabins > 1)
    key = (cellindex * SORT_MABINS) + ((kind == NEXT_KPKT || ma_sub < 0) ? SORT_MABINS - 1 : (ma_sub & (SORT_MABINS - 1)));
#pragma unroll
  for (int k = 1; k < NEXT_NKINDS; k++) {
    int32_t *dst = (k == L.self_kind) ? L.self_list : L.lst[k];
    int32_t *dkey = (k == L.self_kind) ? L.self_key : L.key[k];
    int32_t *cnt = (k == L.self_kind) ? L.self_count : (L.counts + k);
    wave_append(slot == k, pi, key, dst, dkey, cnt);
  }
}
// start of update_packets(): every resident packet is put on the list of its kind. A ContinuumOpacity never survives
// into another call (rpkt.cc:1023 compares globals::timestep; the cell state may have changed in between).
// (Called once per cell-cache tile: only the packets whose cell is in the resident tile are listed, physics.h classify().)
__global__ void __launch_bounds__(BLOCK) k_classify(Env env, Lists L, int reset_chi) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  int kind = NEXT_DONE;
  int32_t cellindex = 0;
  double nu_cmf = 0.;
  if (i < env.P.n) {
    PktHot &h = env.P.hot[i];
    const int type = h.type;
    cellindex = h.cellindex;
    nu_cmf = h.nu_cmf;
    if (reset_chi && h.chi_mgi >= 0) h.chi_mgi = -1;
    const bool active = type_handled(type) && h.prop_time < env.S.ts_end;
    const bool waiting = h.pend != PEND_NONE || h.ma_level >= 0;
    if (active && type_gamma(type) && !waiting) {
      kind = NEXT_GAMMA;
    } else if ((waiting || active) && in_tile(env, cellindex)) {
      if (h.pend != PEND_NONE) {
        kind = NEXT_SLOW;
      } else if (h.ma_level >= 0) {
        kind = NEXT_MA;
      } else if (type == ARTIS_TYPE_RPKT) {
        kind = NEXT_RPKT;
      } else {
        kind = kpkt_blackbody_case(env, type, cellindex) ? NEXT_BB : NEXT_KPKT;
      }
    }
  }
  append_by_kind(kind, (int32_t)i, cellindex, nu_cmf, L);
}

// Adaptive tiles (round 6): how many packets wait in every non-empty cell (the predicate of k_classify, whatever tile is resident), so
// that the next tile can be put where most of them are; *other: packets that need no cache row (gamma-ray kinds, packets in empty cells)
__global__ void __launch_bounds__(BLOCK) k_count_waiting(Env env, int32_t *counts, int32_t *other) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= env.P.n) return;
  const PktHot &h = env.P.hot[i];
  const int type = h.type;
  const bool active = type_handled(type) && h.prop_time < env.S.ts_end;
  const bool waiting = h.pend != PEND_NONE || h.ma_level >= 0;
  if (!(waiting || active)) return;
  const int c = env.M.propcell_nonemptymgi[h.cellindex];
  if ((active && type_gamma(type) && !waiting) || c < 0)
    atomicAdd(other, 1);
  else
    atomicAdd(&counts[c], 1);
}
// ---- counting sort of a work list by its entries' keys (propagation cell, frequency bin).
// Within a cell, r-packets are ordered by comoving frequency like the reference's own packet sort
// (compare_packet_order, update_packets.cc:363): neighbouring lanes then walk the same part of the line list and
// the same window of bound-free continua.
// MANY keys (a 3D grid: cells x bins, millions): two passes whose only atomics are LDS atomics (device-wide atomics on random
// addresses are carried out beyond the XCDs' L2s; one per entry was the whole cost of the sort they replaced).
//  pass 1, by the key's high digit (at most SORT_HI_MAX buckets): k_sort_tilehist counts every tile of SORT_TILE entries in LDS and stores
//    the counts in its column of a [bucket][tile] matrix; the k_scan_* kernels below scan the matrix; k_sort_tilescatter loads a tile's
//    cursors from its scanned column and places (key, entry) pairs, bucket by bucket, in the intermediate buffer.
//  pass 2, by the low digit inside each bucket (a contiguous segment of the intermediate buffer): k_sort_plan cuts the segments into chunks
//    of at most SORT_SEG_CAP entries; k_sort_segments gives every chunk a workgroup that counts the segment's low digits in LDS, scans
//    them there and writes its chunk's entries to their places. A segment of several chunks is counted by each of its workgroups (reads
//    only, from the L2), so a skewed list costs reads, never a workgroup that places a whole bucket on its own.
// Nothing is zeroed per sort, and the scans cover buckets x tiles counters instead of one per key.
constexpr int SORT_HI_BITS = 11;
constexpr int SORT_HI_MAX = 1 << SORT_HI_BITS;
constexpr int SORT_LO_BITS_MAX = 14;  // pass 2's two LDS tables: 2 x 2^14 x 4 B = 128 KB of a workgroup's 160 KB
constexpr int64_t SORT_MAX_KEYS = (int64_t)1 << (SORT_HI_BITS + SORT_LO_BITS_MAX);  // 2^25: a 100^3 grid x SORT_NUBINS
constexpr int SORT_TILE = 8192;     // entries per workgroup of pass 1
constexpr int SORT_TB = 512;
constexpr int SORT_SEG_CAP = 8192;  // entries a workgroup of pass 2 places
__global__ void __launch_bounds__(SORT_TB) k_sort_tilehist(const int32_t *keys, int32_t n, int lobits, int nb, int32_t ntiles, int32_t *mat) {
  __shared__ int32_t h[SORT_HI_MAX];
  for (int b = threadIdx.x; b < nb; b += SORT_TB) h[b] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * SORT_TILE, hi = (lo + SORT_TILE < n) ? lo + SORT_TILE : n;
  for (int64_t i = lo + threadIdx.x; i < hi; i += SORT_TB) atomicAdd(&h[keys[i] >> lobits], 1);
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += SORT_TB) mat[(int64_t)b * ntiles + blockIdx.x] = h[b];
}
// mat: the scanned matrix, mat[b][tile] = where the tile's first entry of bucket b goes
__global__ void __launch_bounds__(SORT_TB) k_sort_tilescatter(const int32_t *list, const int32_t *keys, int32_t n, int lobits, int nb, int32_t ntiles,
                                                              const int32_t *mat, int2 *pairs) {
  __shared__ int32_t h[SORT_HI_MAX];
  for (int b = threadIdx.x; b < nb; b += SORT_TB) h[b] = mat[(int64_t)b * ntiles + blockIdx.x];
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * SORT_TILE, hi = (lo + SORT_TILE < n) ? lo + SORT_TILE : n;
  for (int64_t i = lo + threadIdx.x; i < hi; i += SORT_TB) {
    const int32_t k = keys[i];
    pairs[atomicAdd(&h[k >> lobits], 1)] = make_int2(k, list[i]);
  }
}
// one workgroup: seg[b] = where bucket b begins (seg[nb] = n), chunk_base[b] = chunks of the buckets before it (chunk_base[nb] = all chunks)
__global__ void __launch_bounds__(1024) k_sort_plan(const int32_t *mat, int32_t ntiles, int nb, int32_t n, int32_t *seg, int32_t *chunk_base) {
  __shared__ int32_t part[1024];
  const int t = threadIdx.x;
  int32_t c[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int b = 2 * t + k;
    c[k] = 0;
    if (b < nb) {
      const int32_t s0 = mat[(int64_t)b * ntiles], s1 = (b + 1 < nb) ? mat[(int64_t)(b + 1) * ntiles] : n;
      seg[b] = s0;
      c[k] = (s1 - s0 + SORT_SEG_CAP - 1) / SORT_SEG_CAP;
    }
  }
  if (t == 0) seg[nb] = n;
  part[t] = c[0] + c[1];
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int32_t add = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  const int32_t run = part[t] - c[0] - c[1];
  if (2 * t < nb) chunk_base[2 * t] = run;
  if (2 * t + 1 < nb) chunk_base[2 * t + 1] = run + c[0];
  if (t == 1023) chunk_base[nb] = part[1023];
}
// a workgroup per chunk; sm[]: the segment's count of every low digit, then the cursors; behind it, for a later chunk of a segment, the
// counts of the chunks before it
__global__ void __launch_bounds__(BLOCK) k_sort_segments(const int2 *pairs, int lobits, int nb, const int32_t *seg, const int32_t *chunk_base,
                                                         int32_t *out) {
  extern __shared__ int32_t sm[];
  __shared__ int32_t part[BLOCK];
  __shared__ int s_bucket;
  const int t = threadIdx.x;
  const int nlow = 1 << lobits, mask = nlow - 1;
  if (t == 0) {
    int b = -1;
    if ((int32_t)blockIdx.x < chunk_base[nb]) {  // the last bucket whose chunks begin at or before this one
      int lo = 0, hi = nb - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_base[mid] <= (int32_t)blockIdx.x)
          lo = mid;
        else
          hi = mid - 1;
      }
      b = lo;
    }
    s_bucket = b;
  }
  __syncthreads();
  const int b = s_bucket;
  if (b < 0) return;
  const int32_t s0 = seg[b], s1 = seg[b + 1];
  const int32_t c0 = s0 + ((int32_t)blockIdx.x - chunk_base[b]) * SORT_SEG_CAP, c1 = (s1 - c0 > SORT_SEG_CAP) ? c0 + SORT_SEG_CAP : s1;
  int32_t *tot = sm, *before = sm + nlow;
  const bool later = c0 > s0;
  for (int d = t; d < nlow; d += BLOCK) {
    tot[d] = 0;
    if (later) before[d] = 0;
  }
  __syncthreads();
  for (int32_t i = s0 + t; i < c0; i += BLOCK) {
    const int d = pairs[i].x & mask;
    atomicAdd(&tot[d], 1);
    atomicAdd(&before[d], 1);
  }
  for (int32_t i = c0 + t; i < s1; i += BLOCK) atomicAdd(&tot[pairs[i].x & mask], 1);
  __syncthreads();
  // exclusive scan of tot[]: a run of digits per thread, the threads' sums, the runs again
  const int per = (nlow + BLOCK - 1) / BLOCK;
  const int d0 = (t * per < nlow) ? t * per : nlow, d1 = (d0 + per < nlow) ? d0 + per : nlow;
  int32_t sum = 0;
  for (int d = d0; d < d1; d++) sum += tot[d];
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < BLOCK; off <<= 1) {
    const int32_t add = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int32_t run = part[t] - sum;
  for (int d = d0; d < d1; d++) {
    const int32_t v = tot[d];
    tot[d] = run + (later ? before[d] : 0);
    run += v;
  }
  __syncthreads();
  for (int32_t i = c0 + t; i < c1; i += BLOCK) {
    const int2 p = pairs[i];
    out[s0 + atomicAdd(&tot[p.x & mask], 1)] = p.y;
  }
}
// exclusive scan of a table of counts (the few-keys histogram, the many-keys matrix) in three steps: per-block scan of SCAN_TILE
// counts, scan of the block totals (one block), add the block offsets. A table of one tile is done after the first step.
constexpr int SCAN_TILE = 8192;  // keys per block of 1024 threads (8 per thread)
__global__ void __launch_bounds__(1024) k_scan_tiles(int32_t *hist, int32_t nkeys, int32_t *tile_totals) {
  __shared__ int32_t part[1024];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)t * 8;
  int32_t v[8];
  int32_t sum = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    v[k] = (base + k < nkeys) ? hist[base + k] : 0;
    sum += v[k];
  }
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan of the per-thread sums
    const int32_t add = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int32_t run = part[t] - sum;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (base + k < nkeys) hist[base + k] = run;
    run += v[k];
  }
  if (t == 1023) tile_totals[blockIdx.x] = part[1023];
}
__global__ void __launch_bounds__(1024) k_scan_totals(int32_t *tile_totals, int32_t ntiles) {
  __shared__ int32_t part[1024];
  const int t = threadIdx.x;
  int32_t carry = 0;
  for (int start = 0; start < ntiles; start += 1024) {
    const int i = start + t;
    const int32_t v = (i < ntiles) ? tile_totals[i] : 0;
    part[t] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int32_t add = (t >= off) ? part[t - off] : 0;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    if (i < ntiles) tile_totals[i] = carry + part[t] - v;
    carry += part[1023];
    __syncthreads();
  }
}
__global__ void __launch_bounds__(1024) k_scan_add(int32_t *hist, int32_t nkeys, const int32_t *tile_totals) {
  const int32_t off = tile_totals[blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * 8;
#pragma unroll
  for (int k = 0; k < 8; k++)
    if (base + k < nkeys) hist[base + k] += off;
}
// The same two steps for FEW keys (1D and 2D models, small 3D grids: a few hundred cells). With one global atomic per
// entry the entries of a cell serialise on its counter (measured on a 6^3 grid with 1e7 packets: 7 ms per sort kernel,
// 36 % of the GPU time of a step, against 0.2 ms on the 50^3 grid). Here a workgroup counts its contiguous chunk of the
// list in LDS and touches each global counter once.
constexpr int SORT_LDS_KEYS = 8192;
constexpr int SORT_LDS_GRID = 2048;
__global__ void __launch_bounds__(BLOCK) k_sort_hist_lds(const int32_t *keys, int32_t n, int32_t *hist, int32_t nkeys) {
  __shared__ int32_t h[SORT_LDS_KEYS];
  for (int k = threadIdx.x; k < nkeys; k += BLOCK) h[k] = 0;
  __syncthreads();
  const int64_t chunk = ((int64_t)n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = chunk * blockIdx.x, hi = (lo + chunk < n) ? lo + chunk : n;
  for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) atomicAdd(&h[keys[i]], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < nkeys; k += BLOCK)
    if (h[k] != 0) atomicAdd(&hist[k], h[k]);
}
__global__ void __launch_bounds__(BLOCK) k_sort_scatter_lds(const int32_t *list, const int32_t *keys, int32_t n, int32_t *offsets, int32_t *out,
                                                            int32_t nkeys) {
  __shared__ int32_t h[SORT_LDS_KEYS];
  for (int k = threadIdx.x; k < nkeys; k += BLOCK) h[k] = 0;
  __syncthreads();
  const int64_t chunk = ((int64_t)n + gridDim.x - 1) / gridDim.x;
  const int64_t lo = chunk * blockIdx.x, hi = (lo + chunk < n) ? lo + chunk : n;
  for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) atomicAdd(&h[keys[i]], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < nkeys; k += BLOCK)  // the workgroup's range of each key's output
    if (h[k] != 0) h[k] = atomicAdd(&offsets[k], h[k]);
  __syncthreads();
  for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) out[atomicAdd(&h[keys[i]], 1)] = list[i];
}
inline int sort_lds_grid(int64_t n) {
  const int64_t b = (n + BLOCK - 1) / BLOCK;
  return (int)(b < SORT_LDS_GRID ? b : SORT_LDS_GRID);
}

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

// ---- k_thermal_q (round 5; ARTIS_AMD_REFILL=1): the thermal kernel with the macro-atom walk DECOUPLED from the packet, so that the
// transition loop's lanes are refilled inside the loop. Round 3 built this once (profiles/r03/k_thermal_lane_compaction.md: lanes 35 -> 50,
// and slower, because a transition was then three dependent L2 gathers whose wait grew with the lanes in flight). A transition is now one
// 64-byte sector of the cell's record and two reads of static tables in LDS, and k_thermal runs at 37 of 64 lanes in a loop that is bound
// by instruction issue: re-measured here under today's read pattern.
// A wave owns TQ_V (> 64) packets. What a walk needs of a packet -- generator state, cell, ion's first level, level, counters: 36 B -- is its
// WALK CONTEXT, kept in the wave's LDS slots; the packet's hot line rests in memory meanwhile. Two phases alternate per wave:
//   walk:    every lane holds one context in registers and makes one transition per round; a lane whose walk ends (any process but an
//            internal transition, an undecided search, the launch budget) writes the context back, pushes the slot on the wave's SERVICE
//            stack and pops the next READY slot in the same round (ballot + popcount);
//   service: once 64 slots wait (or the walkers run short), ONE full-wave pass reloads those packets' hot lines, carries out the process
//            that ended each walk (ma_jump_exit), makes the k-packet step that follows, and either prepares the next walk (slot READY, hot
//            line stored) or retires the packet (stored, appended to the list of its next kind) and pulls a new one into the slot.
// Per packet the same functions run in the same order on the packet's own generator as in k_thermal: identical packets, generator states
// and counters (GPU test); estimator sums differ by the order of their additions only.
#ifndef ARTIS_TQ_SLOTS
#define ARTIS_TQ_SLOTS 128
#endif
constexpr int TQ_V = ARTIS_TQ_SLOTS;  // slots per wave: 64 walking + a buffer that lets a full service pass fall due before the walkers starve
static_assert(TQ_V >= 64 && TQ_V <= 256, "slot indices are kept in bytes");
enum { TQ_EMPTY = -2, TQ_BUDGET = -3 };  // action of a slot on the service stack: no packet | walk interrupted by the launch budget
struct TQWave {  // SoA: a lane reads field[its slot]
  uint32_t s0[TQ_V], s1[TQ_V], s2[TQ_V], s3[TQ_V];
  // lv = level within the ion | the ion's first level << 16; cnt = units | njumps << 16; act = (action + 3) | the draw of an undecided search << 7
  int32_t pi[TQ_V], c[TQ_V], lv[TQ_V], cnt[TQ_V];
  uint32_t act[TQ_V];
  uint8_t ready[TQ_V];    // stack of the slots whose walk can go on
  uint8_t service[TQ_V];  // stack of the slots that wait for the service pass
};
template <int TB, bool COLD = false>
__global__ void __launch_bounds__(TB, 1) k_thermal_q(Env env, const int32_t *list, int32_t n, Lists next, unsigned long long *gstats, int budget,
                                                     int32_t *cursors, int nchunks, int drain_budget, int low_water) {
  // dynamic LDS: [TQWave x waves | LevelPack x nlevels | uint16 x nalltrans (padded to words)]
  extern __shared__ __attribute__((aligned(16))) unsigned char tq_lds[];
  __shared__ stat_t lstats[ARTIS_NSTATS];
  TQWave *tq = (TQWave *)tq_lds;
  LevelPack *lds_levelpack = (LevelPack *)(tq_lds + (((sizeof(TQWave) * (TB / 64)) + 15) & ~(size_t)15));
  uint16_t *lds_tlevel = (uint16_t *)(lds_levelpack + env.M.nlevels);
  if (threadIdx.x < ARTIS_NSTATS) lstats[threadIdx.x] = 0;
  for (int i = threadIdx.x; i < env.M.nlevels; i += TB) lds_levelpack[i] = env.M.level_pack[i];
  {
    const uint32_t *src = (const uint32_t *)env.M.alltrans_tlevel16;  // (the allocation is padded to whole words)
    uint32_t *dst = (uint32_t *)lds_tlevel;
    for (int i = threadIdx.x; i < (env.M.nalltrans + 1) / 2; i += TB) dst[i] = src[i];
  }
  env.M.level_pack = lds_levelpack;
  env.M.alltrans_tlevel16 = lds_tlevel;
  env.ma_tables_in_lds = 1;
  env.cellest_lds = nullptr;
  env.cellest_n = 0;
  __syncthreads();
  env.stats = lstats;
  const double ts_end = env.S.ts_end;
  const int lane = threadIdx.x & 63;
  const unsigned long long lanebit = 1ull << lane;
  TQWave &Q = tq[threadIdx.x >> 6];
  Puller q;
  puller_init(q, n, nchunks, 0);
  // wave-uniform stack heights; every slot starts empty and waits for a packet
  int nready = 0, nservice = TQ_V, ndead = 0;
  for (int i = lane; i < TQ_V; i += 64) {
    Q.service[i] = (uint8_t)i;
    Q.act[i] = (uint32_t)(TQ_EMPTY + 3);
  }
  __builtin_amdgcn_wave_barrier();
  bool drained = false;
#ifdef ARTIS_PROFILE
  long long tq_t = clock64();  // wave clocks / 16 of the two phases in the spare stats slots 42 (service) and 43 (walk)
#define TQ_PROF(slot)                                                                   \
  do {                                                                                  \
    const long long now = clock64();                                                    \
    if (lane == 0) atomicAdd(&lstats[slot], (stat_t)((now - tq_t) >> 4));               \
    tq_t = now;                                                                         \
  } while (0)
#else
#define TQ_PROF(slot) ((void)0)
#endif
#if defined(ARTIS_PROFILE) && !defined(ARTIS_PROFILE_MA)
  long long tq_s = clock64();
#define TQ_SUB(slot)                                                                    \
  do {                                                                                  \
    const long long now = clock64();                                                    \
    if (lane == 0) atomicAdd(&lstats[slot], (stat_t)((now - tq_s) >> 4));               \
    tq_s = now;                                                                         \
  } while (0)
#else
#define TQ_SUB(slot) ((void)0)
#endif
  while (true) {
    // ---------------- service passes: while a full wave of slots waits, or the walkers would run short
    while (nservice >= 64 || (nservice > 0 && nready < low_water)) {
#if defined(ARTIS_PROFILE) && !defined(ARTIS_PROFILE_MA)
      tq_s = clock64();
#endif
      const int take = min(64, nservice);
      const bool has = lane < take;
      const int s = has ? (int)Q.service[nservice - 1 - lane] : 0;
      nservice -= take;
      const uint32_t actw = has ? Q.act[s] : (uint32_t)(TQ_EMPTY + 3);
      const int act = (int)(actw & 127u) - 3;
      const bool isdone = has && act != TQ_EMPTY;
      const int32_t idx = pull(q, has && !isdone, cursors);
      if (!drained && q.exhausted) {
        drained = true;
        if (lane == 0) __hip_atomic_store(&cursors[MAX_CHUNKS], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (!drained && drain_budget < budget) drained = __hip_atomic_load(&cursors[MAX_CHUNKS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
      const int budget_now = drained ? drain_budget : budget;
      const bool have = isdone || idx >= 0;
      int32_t pi = 0;
      int units = 0;
      Pkt p;
      MACtx k;
      if (have) {
        pi = isdone ? Q.pi[s] : list[idx];
        pkt_load_thermal(env.P, pi, p);  // the hot line only
        k = ma_ctx(env, p);
        if (isdone) {  // the walk's own state is the slot's; the level's record comes from the static table again
          p.s0 = Q.s0[s]; p.s1 = Q.s1[s]; p.s2 = Q.s2[s]; p.s3 = Q.s3[s];
          const int lv = Q.lv[s];
          p.ma_level = lv & 0xFFFF;
          k.start = lv >> 16;
          k.start_key = (p.ma_element << 8) | p.ma_ion;
          const LevelPack lp = env.M.level_pack[k.start + p.ma_level];
          k.rec = ma_resolve<COLD>(env, k.c, lp.rec_off); k.nd = lp.ndown; k.nu = lp.nup; k.ats = lp.alltrans_startdown;
          const int cnt = Q.cnt[s];
          units = cnt & 0xFFFF;
          k.njumps = cnt >> 16;
          k.defer = (int)(actw >> 7);
        }
      }
#ifdef ARTIS_PROFILE
      if (lane == 0) {
        ARTIS_STAT(env, 47);            // service passes
        ARTIS_STAT_ADD(env, 44, take);  // ... and the slots they served
      }
#endif
      TQ_SUB(59);  // (-DARTIS_PROFILE: wave clocks / 16 of the parts of a service pass: 59 pull + hot line + context | 60 the process that ended
                   //  the walk | 61 the k-packet step | 62 prepare + store + context | 63 classify + append + stacks)
      int kind = NEXT_DONE;
      int32_t out_pi = 0;
      bool walking = false;
      if (have) {  // (one block: split into parts -- as the profile marks would like it -- the compiler spills 93 instead of 13 registers)
        bool go = thermal_can_continue(p, ts_end);
        if (isdone) {
          ma_flush_stats(env, k);
          const U4 *rec = ma_record<COLD>(env, k);
          if (act == MA_EXIT_FILL) {
            p.pend = PEND_MA_FILL;
          } else if (act == MA_EXIT_DEFER) {
            if (!ma_jump_deferred_fine<COLD>(env, p, k, rec)) {
              p.pend = PEND_MA_SEARCH;  // the slow-path kernel re-adds the sums and makes the transition (physics.h ma_slow_search)
              p.pend_arg = k.defer;
            }
          } else if (act >= 0) {
            ma_jump_exit<true>(env, p, pi, k, rec, act);
          }
          chi_after_ma(p);
          go = thermal_can_continue(p, ts_end);
        }
        TQ_SUB(60);
        if (go) {
          // a pre-k-packet, or a k-packet in a grey cell, leaves for the blackbody kernel (classify() below)
          const bool blackbody = (p.type == ARTIS_TYPE_PRE_KPKT) || k.thick;
          if (kpkt_eligible(p, ts_end) && !blackbody) {
            do_kpkt<true>(env, p, pi);
            p.chi_mgi = -1;
            units++;
          }
          go = thermal_can_continue(p, ts_end) && !(blackbody && kpkt_eligible(p, ts_end));
        }
        TQ_SUB(61);
        walking = go && units < budget_now && ma_pending(p) && p.pend == PEND_NONE;
        if (walking) ma_prepare<COLD>(env, p, k);  // (only k.start is kept: the walk phase reads the level's record shape from LDS)
        pkt_store_thermal(env.P, pi, p);  // the hot line; the flight line only if an r-packet was emitted
        if (walking) {
          Q.s0[s] = p.s0; Q.s1[s] = p.s1; Q.s2[s] = p.s2; Q.s3[s] = p.s3;
          Q.pi[s] = pi;
          Q.c[s] = k.c;
          Q.lv[s] = p.ma_level | (k.start << 16);
          Q.cnt[s] = units;
        } else {
          kind = classify(env, p, ts_end);
          out_pi = pi;
        }
      }
      TQ_SUB(62);
      append_by_kind(kind, out_pi, p.cellindex, p.nu_cmf, next, (p.ma_element * 5 + p.ma_ion));
      // where the slots go: READY, or back on the service stack as empty (a packet is pulled into it by the next pass), or --
      // once the work list is used up -- out of use
      {
        const unsigned long long rm = __ballot(walking);
        if (walking) Q.ready[nready + __popcll(rm & (lanebit - 1ull))] = (uint8_t)s;
        nready += __popcll(rm);
        const bool again = has && !walking && !q.exhausted;
        const unsigned long long em = __ballot(again);
        if (again) {
          Q.act[s] = (uint32_t)(TQ_EMPTY + 3);
          Q.service[nservice + __popcll(em & (lanebit - 1ull))] = (uint8_t)s;
        }
        nservice += __popcll(em);
        ndead += take - __popcll(rm) - __popcll(em);
      }
      __builtin_amdgcn_wave_barrier();
      TQ_SUB(63);
    }
    TQ_PROF(42);
    if (nready == 0) break;  // (then nothing waits for service either: every slot is out of use)
    // ---------------- walk phase
    {
      // in the drain (work list used up) a service pass is worth its cost only for a reasonable share of the live slots
      const int drain_min = max(1, min(16, (TQ_V - ndead) / 4));
      const int budget_now = drained ? drain_budget : budget;
      int myslot = -1;
      int units = 0;
      Pkt w;  // only the generator state and ma_level are live
      MACtx k;
      w.ma_level = -1;
      k.c = 0; k.cellma = nullptr; k.rec = 0; k.nd = k.nu = 0; k.ats = 0; k.njumps = 0; k.start = 0; k.start_key = -1; k.defer = 0; k.thick = false;
#ifdef ARTIS_PROFILE
      int prof_rounds = 0, prof_lanes = 0;  // wave-uniform: rounds of this phase and the lanes that made a transition in them
#endif
      while (true) {
        {  // lanes without a context pop READY slots
          const bool need = myslot < 0;
          const unsigned long long m = __ballot(need);
          if (m != 0 && nready > 0) {
            const int takeN = min(__popcll(m), nready);
            const int prefix = __popcll(m & (lanebit - 1ull));
            if (need && prefix < takeN) {
              const int s = (int)Q.ready[nready - 1 - prefix];
              myslot = s;
              w.s0 = Q.s0[s]; w.s1 = Q.s1[s]; w.s2 = Q.s2[s]; w.s3 = Q.s3[s];
              const int lv = Q.lv[s];
              w.ma_level = lv & 0xFFFF;
              k.c = Q.c[s];
              k.cellma = env.K.macache + (krow(env, k.c) * env.M.nmacache);
              k.start = lv >> 16;
              const LevelPack lp = env.M.level_pack[k.start + w.ma_level];
              k.rec = ma_resolve<COLD>(env, k.c, lp.rec_off); k.nd = lp.ndown; k.nu = lp.nup; k.ats = lp.alltrans_startdown;
              const int cnt = Q.cnt[s];
              units = cnt & 0xFFFF;
              k.njumps = cnt >> 16;
            }
            nready -= takeN;
          }
        }
        const int nactive = __popcll(__ballot(myslot >= 0));
        if (nactive == 0 || nservice >= 64 || (nactive < low_water && nservice >= drain_min)) break;
        bool ended = false;
        int end_action = 0;
        {
          const bool go = myslot >= 0;
#ifdef ARTIS_PROFILE
          prof_lanes += __popcll(__ballot(go));
          prof_rounds++;
#endif
          if (go) {
            const int action = ma_jump_internal<true, COLD>(env, w, k, ma_record<COLD>(env, k));
            units++;
            if (action >= 0 || units >= budget_now) {
              ended = true;
              end_action = action >= 0 ? action : TQ_BUDGET;
            }
          }
        }
        const unsigned long long em = __ballot(ended);
        if (em != 0) {
          if (ended) {
            const int s = myslot;
            Q.s0[s] = w.s0; Q.s1[s] = w.s1; Q.s2[s] = w.s2; Q.s3[s] = w.s3;
            Q.lv[s] = w.ma_level | (k.start << 16);
            Q.cnt[s] = units | (k.njumps << 16);
            Q.act[s] = (uint32_t)(end_action + 3) | ((uint32_t)k.defer << 7);
            Q.service[nservice + __popcll(em & (lanebit - 1ull))] = (uint8_t)s;
            myslot = -1;
          }
          nservice += __popcll(em);
        }
      }
      // park the walks in progress: their slots are READY again
      const bool parked = myslot >= 0;
      const unsigned long long pm = __ballot(parked);
      if (parked) {
        const int s = myslot;
        Q.s0[s] = w.s0; Q.s1[s] = w.s1; Q.s2[s] = w.s2; Q.s3[s] = w.s3;
        Q.lv[s] = w.ma_level | (k.start << 16);
        Q.cnt[s] = units | (k.njumps << 16);
        Q.ready[nready + __popcll(pm & (lanebit - 1ull))] = (uint8_t)s;
      }
      nready += __popcll(pm);
#ifdef ARTIS_PROFILE
      if (lane == 0) {
        ARTIS_STAT_ADD(env, 46, prof_rounds);  // wave-rounds of the transition loop
        ARTIS_STAT_ADD(env, 45, prof_lanes);   // ... and the lanes that made a transition in them
      }
#endif
      __builtin_amdgcn_wave_barrier();
      TQ_PROF(43);
    }
  }
  __syncthreads();
  if (threadIdx.x < ARTIS_NSTATS && lstats[threadIdx.x] != 0) atomicAdd(&gstats[threadIdx.x], lstats[threadIdx.x]);
}
#ifndef ARTIS_TQ_TB
#define ARTIS_TQ_TB 768
#endif
constexpr int TQ_TB = ARTIS_TQ_TB;  // 12 waves per CU = 3 waves/SIMD at 168 VGPRs (round 3's optimum for this form; the slots of 16 waves and the tables do not fit the LDS)
inline size_t tq_lds_bytes(int tb, int nlevels, int nalltrans) {
  return (((sizeof(TQWave) * (size_t)(tb / 64)) + 15) & ~(size_t)15) + (sizeof(LevelPack) * (size_t)nlevels) + (sizeof(uint32_t) * (size_t)((nalltrans + 1) / 2));
}

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

inline int nblocks(int64_t n) { return (int)((n + BLOCK - 1) / BLOCK); }

// the timestep-end stages (stage_*.h, included at the end of this file); the engine holds each one's state from its first call on
struct SpecState;
void spec_free(SpecState *st);
struct RfState;
void rf_free(RfState *st);
struct IbState;
void ib_free(IbState *st);
struct DecayState;
void decay_free(DecayState *st);
struct DepState;
void dep_free(DepState *st);
struct PinitState;
void pinit_free(PinitState *st);
struct TbState;
void tb_free(TbState *st);
struct BfhState;
void bfh_free(BfhState *st);
struct RcState;
void rc_free(RcState *st);
struct PiState;
void pi_free(PiState *st);

}  // namespace

// ------------------------------------------------------------------ engine object
// What one artis_amd_update_packets_device call did: zeroed when the call begins, read by the artis_amd_last_* accessors.
struct LastCall {
  double propagate_ms = 0., kms[NEXT_NKINDS] = {}, kms_tail = 0., fill_ms = 0.;  // summed launch durations: all, per kind, the tail kernel's; tile fills'
  double kms_late = 0.;          // ... k_late's
  int64_t late_launches = 0, tail_launches = 0;
  int64_t late_bailouts = 0;     // waves of k_late that gave up waiting for work (ARTIS_AMD_TRACE prints them)
  int64_t klaunches[NEXT_NKINDS] = {}, kthreads[NEXT_NKINDS] = {}, nlaunches = 0;
  // tiled runs: sweeps over the tiles, tile fills (sparse ones, cells filled), packets listed per (sweep, tile), packets parked
  int64_t sweeps = 0, tile_fills = 0, sparse_fills = 0, cells_filled = 0, listed = 0, parked = 0;
  int64_t pool_resets = 0;       // times the pool of on-demand records was emptied because it was used up
  int32_t thermal_variants = 0, est_forms = 0;  // thermal-kernel instantiations launched; how the kernels added to the per-cell estimators (include/artis_amd.h)
};
// what the many-keys sort of a list of up to `capacity` entries needs besides its input and output: one allocation
struct SortScratch {
  void *base = nullptr;
  int64_t capacity = 0;
  int2 *pairs = nullptr;          // [capacity] pass 1's output: (key, entry), bucket by bucket
  int32_t *mat = nullptr;         // [SORT_HI_MAX][tiles of the list] the tiles' bucket counts, scanned in place
  int32_t *tiles = nullptr;       // the scan's tile totals
  int32_t *seg = nullptr;         // [SORT_HI_MAX + 1] where every bucket begins
  int32_t *chunk_base = nullptr;  // [SORT_HI_MAX + 1] pass 2's chunks before every bucket
};
// The cell cache's host state: which cells hold rows (cache_residency.h), the device copies of that, and what a fill works on and with (stage_cellcache.h).
struct CellCache {
  // Cell-cache tiling: the cache rows of `res.tile_cells` non-empty cells are resident at a time (all of them when they fit
  // the budget: ntiles == 1). With more tiles, update_packets sweeps over them -- populate a tile, advance every packet
  // that sits in one of its cells until it leaves the tile or is done -- until no packet is left (what the reference's
  // single-slot cell cache does cell by cell, update_packets.cc:397-460, 551-621).
  int ntiles = 1;
  int tile_lo = 0, tile_hi = 0;   // one tile: all cells (the range a whole-cache fill works on)
  int tile_valid_lo = -1;         // one tile: 0 once the cache is populated for the current cell state (-1: not)
  // several tiles: which cell's cache each row holds, populated for the current cell state (physics.h Env::krow_tab; make_resident())
  artis_residency::Residency res;
  int32_t *d_krow = nullptr;         // the device's copy of res.krow
  std::vector<int32_t> h_cell_grid;  // [npts_nonempty] the grid cell of a non-empty cell (the inverse of propcell_nonemptymgi)
  size_t cache_bytes_per_cell = 0;
  // the cells a fill of a tiled cache works on (make_resident()). Sparse fills: a visit for which few packets wait makes the cells in which they
  // wait (and the cells around those) resident instead of a whole window. ARTIS_AMD_SPARSE_FILL=0: whole windows.
  int32_t *d_fill_cells = nullptr;
  bool sparse_fill = true;
  int64_t sparse_max_listed = 16384;  // ... for visits that list at most this many packets (ARTIS_AMD_SPARSE_MAX; 512 in round 3:
                                      // 4 tiles 3327 / 3205 / 3188 ms at 512 / 4096 / 16384, with parked tails 3222 / 3123 / 2982)
  // Adaptive tiles (round 6; ARTIS_AMD_TILE_ADAPT=0: the fixed ranges of rounds 2-5). WHICH cells are resident is chosen before every visit from
  // the number of packets that wait in every cell (k_count_waiting): the window of tile_cells consecutive cells in which most packets wait
  // (ARTIS_AMD_TILE_BLOCK=0), or the blocks of tile_block consecutive cells in which most wait, wherever they lie (a tile = a SET of cells: rows are
  // addressed through Env::krow_tab). A cell that is resident and still wanted keeps its row -- only the cells that are new to the set are filled.
  // The first visits take the densest parts of the ejecta; afterwards the waiting packets sit on both sides of the earlier sets' edges, and a set laid
  // across such an edge lets them cross it freely instead of waiting once per crossing and fixed tile.
  bool tile_adapt = true;
  int64_t tile_block = 0;
  bool pool_keep = true;
  int32_t *d_waiting = nullptr;  // [npts_nonempty + 1] packets waiting per cell; the last entry: packets that need no row
  std::vector<int32_t> h_waiting;
  // the population's scratch: the collisional-excitation cooling terms of `pop_batch` cells at a time (k_matrans writes them,
  // k_cooling_chain turns them into running sums, k_collexc_filter into the records' cooling filters; nothing of it is kept)
  double *d_collexc_terms = nullptr;
  int64_t pop_batch = 0;
};
struct artis_amd_engine {
  int device = 0;
  EngineConfig cfg;           // the resolved configuration (engine_config.h resolve_config: struct field, else ARTIS_AMD_* variable, else default)
  double cache_budget = 0.;   // [B] the budget the rows were sized by (given, or the automatic rule on the free memory at creation)
  SpecState *spec = nullptr;  // artis_amd_spectra_*: nothing until the first call
  RfState *rf = nullptr;      // artis_amd_radfield_*: nothing until the first call
  IbState *ib = nullptr;      // artis_amd_grid_update*: nothing until the first call
  DecayState *decay = nullptr;  // artis_amd_decay_*: nothing until artis_amd_decay_setup
  DepState *dep = nullptr;      // artis_amd_deposition_*: nothing until artis_amd_deposition_setup
  PinitState *pinit = nullptr;  // artis_amd_packet_init*: nothing until artis_amd_packet_init_setup
  TbState *tb = nullptr;        // artis_amd_thermal_*: nothing until the first call
  BfhState *bfh = nullptr;      // artis_amd_bfheating_*: nothing until the first call
  RcState *rc = nullptr;        // artis_amd_ratecoeff_*: nothing until the first call
  PiState *pi = nullptr;        // artis_amd_set_cellstate_photoion: nothing until the first call
  double *pi_coeff = nullptr;   // ... its coefficients [cell][nphixstargets_total] among cell_allocs (null: the cell state is not of that call)
  uint64_t cellstate_serial = 0;  // counts the changes of the resident cell state (artis_amd_set_cellstate, the hand-over of artis_amd_grid_update*)
  bool fit_since_step = false;  // an artis_amd_radfield_fit since the last propagation call (artis_amd_grid_update use_fit)
  ModelOwned own;
  std::vector<void *> model_allocs;
  std::vector<void *> cell_allocs;
  std::vector<void *> cache_allocs;
  DevModel M{};  // device pointers
  DevModel Mh{};  // host view (counts)
  artis_model model_copy{};                        // sizes + level_matransblock_start kept for diagnostics
  std::vector<int32_t> own_matransblock_start;
  DevCells C{};
  DevCache K{};
  DevStep S{};
  DevEst E{};
  bool have_cells = false;
  bool expopac_own = false;  // the expansion-opacity tables are the engine's (calculated at cell-cache population)
  BfEvent *d_bfev = nullptr;     // deferred bound-free estimator updates of one k_rpkt launch (DETAILED_BF builds)
  int32_t *d_bfev_count = nullptr;
  // the sums of the deferred updates, [cell][place in the cell's list of kept continua]: the additions of a record go to
  // neighbouring doubles instead of ~30 separate 64-byte sectors of bfrate_raw; k_bfrate_expand moves them when a call ends
  double *d_bfrate_kept = nullptr;
  bool bfrate_kept_dirty = false;  // a call ended in an error before its sums were moved
  int32_t bfev_cap = 0;
  bool bf_defer = true;          // ARTIS_AMD_BFDEFER=0: add in place inside k_rpkt
  // virtual packets (VPKT_ON builds): the configuration block, and the events one launch records for k_vpkt (at most
  // budget_r per packet on the launch's list: an electron scattering per do_rpkt_step(), one emission per thermal visit)
  VpktConfig *d_vpkt_config = nullptr;
  VpktSeed *d_vpkt_queue = nullptr;
  int32_t *d_vpkt_count = nullptr;
  int32_t vpkt_cap = 0;
  CellCache cc;  // the cell cache: which cells hold rows, what a fill works on (stage_cellcache.h)
  int32_t *d_target_level = nullptr;
  double *d_est = nullptr;
  int64_t est_ndoubles = 0;
  int64_t nvspec = 0, nvgrid = 0;  // doubles of the virtual-packet spectra / velocity-grid map at the end of the block
  unsigned long long *d_stats = nullptr;
  int32_t *d_err = nullptr;      // (the slot after the list counters: one copy brings both to the host)
  int32_t *h_counts = nullptr;   // pinned: the host's copy of the list counters and the error flag after every launch
  // packets
  int64_t npackets = -1;           // -1: no resident population
  void *d_pkt = nullptr;           // the three record arrays of the resident population (tables.h PktStore)
  void *d_pkt_snapshot = nullptr;
  size_t pkt_bytes = 0;
  PktStore P{};
  artis_packet *d_aos = nullptr;
  int64_t aos_capacity = 0;
  bool aos_valid = false;  // d_aos still holds the caller's structs of the resident population (set by the upload)
  int32_t *d_lists[NEXT_NKINDS][2] = {};      // per kind: current and alternate work list
  int32_t *d_keys[NEXT_NKINDS][2] = {};       // ... and the sort keys of their entries
  int32_t *d_sorted = nullptr;                // counting-sort output
  int32_t *d_perm = nullptr;                  // record slot -> index in the caller's packet array (k_aos_to_rec)
  bool use_perm = false;                      // d_perm describes the resident population
  bool slot_order_by_cell = true;             // ARTIS_AMD_SLOTSORT=0: slots in the caller's order
  int32_t *d_hist = nullptr;                  // [SORT_LDS_KEYS + 1] key histogram of the few-keys sort
  int32_t *d_tiles = nullptr;                 // ... and its scan's tile totals
  SortScratch sort_scratch;                   // the many-keys sort's buffers, allocated with the lists
  bool sort_attr_set = false;                 // k_sort_segments may use its 128 KB of LDS on this engine's device
  int32_t *d_count = nullptr;                 // [NEXT_NKINDS] current-list counts, [NEXT_NKINDS] alternate-list count
  int32_t *d_cursors = nullptr;               // [PULL_SLOTS] chunk cursors of the running pull kernel (work_pull.h)
  int ncu = 256;
  double *d_gamma_ws = nullptr;   // per-packet groundcont_gamma_contr lists (physics.h Env)
  int32_t *d_gamma_gi = nullptr;
  int32_t *d_gamma_n = nullptr;
  int64_t ws_capacity = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  LastCall last;  // what the last artis_amd_update_packets_device call did (artis_amd_last_*)
  // (builds with the detailed bound-free estimators -- the nltenebular family -- alternate twice as often between the
  // kernels and their r-packet steps are ~3x as heavy: measured optimum 16384 / 4 / 1024 instead of 4096 / 8 / 2048,
  // nltenebular step 1801 -> 1690 ms, profiles/r03/neb_sweep*.txt)
  int tail_max = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? 16384 : 4096;  // r-packets + thermal packets left at which k_tail takes over (artis_amd_config.tail_threshold; 0 = never)
  bool tail_always = false;           // ... also for a population that starts below it (ARTIS_AMD_TAIL_ALWAYS=1)
  // k_late: r-packets + thermal packets left at which one persistent launch takes over from the split kernels (ARTIS_AMD_LATE; 0 = never;
  // chosen by a sweep on the headline, profiles/r08/late_kernel.md), for a population that began larger -- or any (ARTIS_AMD_LATE_ALWAYS=1)
  int64_t late_max = 200000;
  bool late_always = false;
  bool late_strict = false;           // ARTIS_AMD_LATE_STRICT=1: a wave of k_late that gave up waiting fails the call (tests)
  bool late_attr_set = false;         // k_late's dynamic-LDS attribute has been set on this engine's device
  int32_t *d_late_ring[LATE_NQ] = {nullptr, nullptr, nullptr};  // the workgroups' queues (allocated with the lists)
  int32_t *d_late_bail = nullptr;     // the slot after the error flag
#ifdef ARTIS_PROFILE_LATE
  int32_t *d_late_stamp = nullptr;    // (k_late's profile: LateArgs::stamp; lives as long as the process)
#endif
  bool park_tails = true;     // ARTIS_AMD_TILE_PARK=0: every visit of a tile runs its packets to their end (rounds 2-3)
  // artis_amd_config.tile_park_at: packets left of a larger visit at which it parks them (0 / <= tail_max: round 4's rule, at the tail kernel's
  // threshold). Measured on the headline at a quarter of its cache (4 tiles, adaptive windows; profiles/r06/tiling.md): 4096 / 32768 / 131072 /
  // 524288 / 2097152 -> 2395 / 2147 / 1971 / 1899 / 1868 ms per step (untiled 760); with this round's rows for sets of cells and record tiers (two tiles
  // of rows with a quarter of the levels hot): 131072 / 524288 / 2097152 / 3145728 / 4194304 -> 1550 / 1532 / 1504 (1485 on the box of the last two) / 1448 / 1452 ms;
  // three tiles at 11600 MB: 2097152 / 3145728 / 4194304 -> 1590 / 1573 / 1670 ms
  int64_t park_at = 3145728;
  int64_t last_pool_used = 0, last_pool_cap = 0;  // units (128 B) of the pool in use at the end of the last call that had cold levels / its size (no call resets them)
  double ma_hotfrac = 1.;        // the share of every ion's levels that has a static record (given, or chosen by engine_fill from the cache budget)
  bool vpkt_cont_lds = true;  // ARTIS_AMD_VPKT_CONTLDS=0: k_vpkt reads the continuum table from memory (four workgroups of 256 per CU)
  bool tile_zigzag = false;  // ARTIS_AMD_TILE_ZIGZAG=1: sweeps alternate their direction (measured slower: profiles/r03/tiling.md)
  int64_t last_visits = 0;  // visits of the last call that had packets (the driver's own count: adaptive tiles, trace)
  // do_rpkt_step() calls per packet per launch. 8 in rounds 2-3; with the r-packet kernel's reads requested ahead (round 4) the list's order
  // -- sorted by cell and frequency before every launch -- is worth more than the launches saved: 857 / 855 / 851 / 846 / 860 / 881 ms per step
  // at 8 / 6 / 5 / 4 / 3 / 2 (classic; kilonova_lte 859 / 844 / 858 at 8 / 4 / 3; nltenebular, 4 since round 3: 1199 / 1204 / 1235 at 4 / 3 / 2)
  // (8 stays where a step is cheap and launches are not: the expansion-opacity build with thermalising bound-bound events, 520 vs 567 ms,
  // and the virtual-packet builds, whose every launch is followed by k_vpkt: 1250 vs 1268 ms)
  int budget_r = (ARTIS_OPT_RPKT_BB_THERMALISATION || ARTIS_OPT_VPKT_ON) ? 8 : 4;
  int budget_g = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? 32 : 64;      // ... of a gamma packet (k_gamma)
  int budget_t = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? 1024 : 2048;  // macro-atom transitions / k-packet steps per packet per launch
  // A launch lasts as long as its slowest packet, and a list that does not fill the GPU any more (the last tenth of a
  // timestep's rounds) is bound by that alone. Smaller budgets for such lists (ARTIS_AMD_SMALL_LIST, ARTIS_AMD_BUDGET_T_SMALL /
  // _R_SMALL; 0 = off, the default) were measured: classic 1160 -> 1182..1258 ms per step (the extra rounds cost more than
  // the shorter launches save), nltenebular 1500 -> 1481 (profiles/r03/small_list_budgets.txt).
  int small_list = 300000;
  int budget_t_small = 0;
  int budget_r_small = 0;
  // k_thermal's unit budget while its list still has entries, in launches with the hand-over at list exhaustion below (EngineConfig::budget_t_bulk,
  // ARTIS_AMD_BUDGET_T_BULK; 0 = none). None: the wave's other lanes keep pulling beside a long history and the hand-over ends the launch anyway, so
  // budget_t there only stored, listed, sorted and loaded such a packet again every round. Launches without hand-over keep budget_t.
  int budget_t_bulk = 0;
  // ... and after the launch's list is used up (ARTIS_AMD_DRAIN_T; 0 = off), in launches of at least drain_min_list packets
  int drain_t = 48;
  int drain_r = 1;       // ... do_rpkt_step() calls after the r-packet list is used up (ARTIS_AMD_DRAIN_R; 0 = off)
  int64_t drain_min_list = 1000000;
  bool sort_lists = true;
  bool sort_nu = true;
  // The r-packet list sorted by (frequency bin, cell) instead of (cell, frequency bin) (round 5; ARTIS_AMD_SORT_NUMAJOR=0: rounds 2-4): the
  // 64 packets a wave holds then lie in one of 32 frequency bins (four per octave) -- their opacity sums run over windows of similar length
  // and their line walks through the same stretch of the line list -- and in ~7 neighbouring cells of it. k_rpkt 263 -> 251 ms with 16 bins,
  // 244 with 32, 245 with 64, 250 with 128 (MI355X, headline workload; profiles/r05/sort_numajor.txt).
  bool sort_numajor = true;
  int sort_cellshift = 0;  // ARTIS_AMD_SORT_CELLSHIFT (with the frequency bin as the major part only)
  bool sort_ma = true;
  // lists with more entries per cell of the tile than this are not sorted (sort_by_key) unless the kernel accumulates its
  // per-cell estimators in LDS; measured crossover of the thermal lists with 1e7 packets: between 20^3 and 30^3 cells
  // (1 250 / 370 per cell). ARTIS_AMD_SORT_MAXPC_R / _T.
  // 512 < cells <= 3072: k_rpkt keeps J / nuJ / ffheating in LDS instead of the continuum table (12^3 grid, 912 cells:
  // k_rpkt 292 -> 215 ms; 14^3, 1472 cells: 249 -> 225 ms). ARTIS_AMD_RPKT_EST_OVER_CONT=0: the table wins the LDS.
  bool rpkt_est_over_cont = true;
  int ma_bins = SORT_MABINS;    // the thermal list sorted by (cell, a hash of the macro-atom's ion) instead of by cell alone: the lanes of a wave
                                // start in the records of one or two ions (ARTIS_AMD_MABINS=1: by cell; step 1060 -> ~1050 ms)
  bool ma_filters = true;       // macro-atom transitions decided on the records' 15-bit filters (ARTIS_AMD_MAFILTERS=0: on the f64 values)
  int dense_lpr = 32;           // k_bfest_dense: lanes per record (64 = a wave per record; ARTIS_AMD_DENSE_LPR)
  bool dense_cont_lds = true;   // k_bfest_dense reads the continuum table from LDS (nltenebular step 1917 -> 1882 ms); ARTIS_AMD_DENSE_CONTLDS=0
  bool cellest_in_lds = true;  // ARTIS_AMD_CELLEST_LDS=0: every estimator add is a global atomic
  bool estcache = true;        // ARTIS_AMD_ESTCACHE=0: k_rpkt without its waves' caches of per-cell accumulators (physics.h Env::estcache)
  int sort_maxpc_r = 20000;
  int sort_maxpc_t = 600;
  // one list chunk per wave instead of one per XCD (artis_engine.hip pull): measured on MI355X, 1e7 packets: k_rpkt -4 %
  // (a wave's lanes share continuum windows and line ranges), k_thermal +30 % (every wave then has its own cells in
  // flight and the L2 working set of macro-atom records triples)
  bool wave_chunks_r = true, wave_chunks_t = false;
  bool cu_chunks_t = false;  // ARTIS_AMD_CUCHUNKS_T=1: k_thermal takes one list chunk per compute unit (HW_REG_HW_ID);
                             // measured +7 %: like every finer chunking it puts more cells in flight per XCD
  bool cont_lds = true;      // k_rpkt keeps the static continuum table (ContPack) in LDS when it fits (ARTIS_AMD_CONTLDS=0: HBM)
  bool line_lds = false;     // ARTIS_AMD_LINELDS=1: the line list's frequencies in LDS instead (k_rpkt<false, .., true>; measured slower)
  int thermal_blocks_per_cu = ARTIS_THERMAL_WAVES;  // tuning: resident k_thermal blocks per CU
  bool thermal_refill = false;  // ARTIS_AMD_REFILL=1: k_thermal_q (walk contexts in per-wave LDS slots, lanes refilled inside the transition loop)
  int tq_low = 48;              // ... its low-water mark of walking lanes (ARTIS_AMD_TQ_LOW)
  bool tq_attr_set = false;     // ... its dynamic-LDS attribute has been set on this engine's device
  bool ma_tables_lds = true;  // k_thermal<1024, true>: the static target tables in LDS when they fit (ARTIS_AMD_MATABLES_LDS=0: in HBM)
  bool trace = false;
  uint32_t *d_visit_counts = nullptr;  // -DARTIS_VISIT_COUNTS builds: [cell][level] transitions drawn per record in the last call
  // ABSENT IONS (tables.h; EngineConfig::ma_absent_eps >= 0): [resident row][nions] the ions whose static records the last population of the row left
  // out, and the two counters behind artis_amd_last_absent_records(): records left out by the last population | filled on demand in the last call
  uint8_t *d_ion_absent = nullptr;
  double *d_ion_popsum = nullptr;  // k_ion_absent's scratch, [resident row][nions]
  unsigned long long *d_absent_counts = nullptr;
  int64_t last_absent_skipped = 0, last_absent_filled = 0;
  ncclComm_t comm = nullptr;  // created by artis_amd_comm_init(), owned by the engine
};

// The configuration of an engine, resolved once (engine_config.h resolve_config: struct field, else ARTIS_AMD_* variable, else default) into e->cfg, which
// the sizing code reads, and into the driver's fields. Called by artis_amd_engine_create_ex before anything is sized; no other place reads these variables.
static void apply_config(artis_amd_engine *e, const artis_amd_config &checked) {
  e->cfg = resolve_config(checked);
  if (e->cfg.tail_given) e->tail_max = e->cfg.tail_threshold;
  if (ARTIS_OPT_VPKT_ON) e->tail_max = 0;  // (see the estimator block: the event queue is sized per split launch)
  if (e->cfg.park_given) e->park_at = e->cfg.tile_park_at;
  if (e->cfg.bulk_given) e->budget_t_bulk = e->cfg.budget_t_bulk;
  // ABSENT IONS: off by default in the builds with non-thermal ionisation (the nebular family) -- their macro-atoms reach sparsely populated ions
  // through the non-thermal channels, 3.1e5 fills per headline step at eps = 1e-12, and the step is 27 ms longer (profiles/r12/absent_ions.md);
  // ARTIS_AMD_MA_ABSENT_EPS turns it on
  if (ARTIS_OPT_NT_ON && e->cfg.src_absent == CONFIG_DEFAULT) e->cfg.ma_absent_eps = -1.;
}
static void trace_config(const artis_amd_engine *e) {
  const EngineConfig &c = e->cfg;
  fprintf(stderr,
          "[artis_amd] configuration: cache_budget_bytes %.0f (%s), cache_headroom_bytes %.0f (%s), pop_scratch_bytes %.0f (%s), ma_hot_fraction %.3f (%s), "
          "ma_pool_fraction %.3f (%s), tail_threshold %d (%s), tile_park_at %lld (%s), keep_line_dpop %d (%s)\n",
          e->cache_budget, c.budget_given ? config_source_name(c.src_budget) : "default: automatic", c.cache_headroom, config_source_name(c.src_headroom),
          c.pop_scratch, config_source_name(c.src_scratch), e->ma_hotfrac, c.hot_given ? config_source_name(c.src_hot) : "default: automatic", c.ma_pool,
          config_source_name(c.src_pool), e->tail_max, config_source_name(c.src_tail), (long long)e->park_at, config_source_name(c.src_park),
          e->Mh.ndpop > 0 ? 1 : 0, c.keep_line_dpop >= 0 ? config_source_name(c.src_dpop) : "default: automatic");
  fprintf(stderr, "[artis_amd] absent ions: ARTIS_AMD_MA_ABSENT_EPS %g (%s)%s\n", c.ma_absent_eps, config_source_name(c.src_absent),
          e->d_ion_absent != nullptr ? "" : ": every static record is populated");
}

// The experiment switches (ARTIS_AMD_*: kernel forms, sorts, chunking) of the fields above (engine_fill). Order: BUDGET before _R / _T, SORT_CELLSHIFT after SORT_NUMAJOR.
static void read_switches(artis_amd_engine *e) {
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET")) {  // tuning / tests: launch budgets never change results
    e->budget_r = std::max(1, std::atoi(b));
    e->budget_t = std::max(1, std::atoi(b));
    e->budget_g = e->budget_r * 8;
  }
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_R")) e->budget_r = std::max(1, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_T")) e->budget_t = std::max(1, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_SMALL_LIST")) e->small_list = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_T_SMALL")) e->budget_t_small = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_BUDGET_R_SMALL")) e->budget_r_small = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_DRAIN_T")) e->drain_t = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_DRAIN_R")) e->drain_r = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_DRAIN_MIN")) e->drain_min_list = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_SLOTSORT")) e->slot_order_by_cell = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_BFDEFER")) e->bf_defer = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT")) e->sort_lists = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_NU")) e->sort_nu = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_MA")) e->sort_ma = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TAIL_ALWAYS")) e->tail_always = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_LATE")) e->late_max = std::max<int64_t>(0, std::atoll(b));
  if (const char *b = std::getenv("ARTIS_AMD_LATE_ALWAYS")) e->late_always = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_LATE_STRICT")) e->late_strict = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_RPKT_EST_OVER_CONT")) e->rpkt_est_over_cont = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_DENSE_CONTLDS")) e->dense_cont_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_MABINS")) e->ma_bins = (std::atoi(b) > 1) ? SORT_MABINS : 1;
  if (const char *b = std::getenv("ARTIS_AMD_MAFILTERS")) e->ma_filters = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_DENSE_LPR")) e->dense_lpr = (std::atoi(b) == 64) ? 64 : (std::atoi(b) == 16 ? 16 : 32);
  if (const char *b = std::getenv("ARTIS_AMD_CELLEST_LDS")) e->cellest_in_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_ESTCACHE")) e->estcache = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_MAXPC_R")) e->sort_maxpc_r = std::max(1, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_SORT_MAXPC_T")) e->sort_maxpc_t = std::max(1, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_WAVECHUNKS_R")) e->wave_chunks_r = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_WAVECHUNKS_T")) e->wave_chunks_t = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_CUCHUNKS_T")) e->cu_chunks_t = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_CONTLDS")) e->cont_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_LINELDS")) e->line_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TILE_ZIGZAG")) e->tile_zigzag = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TILE_ADAPT")) e->cc.tile_adapt = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TILE_BLOCK")) e->cc.tile_block = std::max<int64_t>(0, std::atoll(b));
  if (const char *b = std::getenv("ARTIS_AMD_POOL_KEEP")) e->cc.pool_keep = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_MATABLES_LDS")) e->ma_tables_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_REFILL")) e->thermal_refill = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_NUMAJOR")) e->sort_numajor = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SORT_CELLSHIFT")) e->sort_cellshift = e->sort_numajor ? std::max(0, std::min(20, std::atoi(b))) : 0;
  if (const char *b = std::getenv("ARTIS_AMD_TQ_LOW")) e->tq_low = std::max(1, std::min(64, std::atoi(b)));
  if (const char *b = std::getenv("ARTIS_AMD_SPARSE_FILL")) e->cc.sparse_fill = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_SPARSE_MAX")) e->cc.sparse_max_listed = std::max(0, std::atoi(b));
  if (const char *b = std::getenv("ARTIS_AMD_THERMAL_BLOCKS")) e->thermal_blocks_per_cu = std::max(1, std::min(ARTIS_THERMAL_WAVES, std::atoi(b)));
  e->trace = std::getenv("ARTIS_AMD_TRACE") != nullptr;
  if (const char *b = std::getenv("ARTIS_AMD_VPKT_CONTLDS")) e->vpkt_cont_lds = std::atoi(b) != 0;
  if (const char *b = std::getenv("ARTIS_AMD_TILE_PARK")) e->park_tails = std::atoi(b) != 0;
}

namespace {

template <typename T>
int upload_array(std::vector<void *> &allocs, const T *host, int64_t count, const T **dev_out) {
  T *d = nullptr;
  const size_t bytes = sizeof(T) * (size_t)(count > 0 ? count : 1);
  HIP_TRY(hipMalloc((void **)&d, bytes));
  allocs.push_back(d);
  if (count > 0) HIP_TRY(hipMemcpy(d, host, sizeof(T) * (size_t)count, hipMemcpyHostToDevice));
  *dev_out = d;
  return ARTIS_OK;
}

int free_all(std::vector<void *> &v) {
  for (void *p : v) (void)hipFree(p);
  v.clear();
  return ARTIS_OK;
}

Env make_env(const artis_amd_engine *e) {
  Env env;
  std::memset(&env, 0, sizeof(env));
  env.M = e->M;
  env.C = e->C;
  env.K = e->K;
  {
    const DevModel &h = e->Mh;
    if (h.ndpop == 0) env.K.line_dpop = nullptr;  // formed on the fly (physics.h line_dpop_at)
    // the pool of on-demand records is one for all resident cells (tables.h "ON-DEMAND RECORDS"): not indexed by cell
    env.ma_pool_cap = (uint32_t)std::min<int64_t>(((int64_t)e->cc.res.tile_cells * h.ma_pool_slots) / MAPOOL_UNIT, 0x7FFFFFF0LL);
    env.ma_pool_full = e->d_count + (2 * NEXT_NKINDS - 1);  // (a spare slot of the counts the host reads after every launch)
  }
  // rows: one per cell (row = cell), or -- a cache that does not fit -- the rows of the cells that are resident now (make_resident())
  env.krow_tab = e->cc.ntiles > 1 ? e->cc.d_krow : nullptr;
  env.tile_all = e->cc.ntiles > 1 ? 0 : 1;
  env.tile_lo = 0;
  env.tile_hi = e->Mh.npts_nonempty;
  env.fill_cells = nullptr;  // (set by populate_tile() of a tiled cache for its own launches)
  env.nfill = 0;
  env.collexc_terms = e->cc.d_collexc_terms;
  {  // few cells: per-cell estimators accumulate in LDS (physics.h Env::cellest_lds)
    const int nc = e->Mh.npts_nonempty;
    env.cellest_n_t = (e->cellest_in_lds && nc <= THERMAL_CELLEST_CAP) ? nc : 0;
    // between the two caps k_rpkt runs without the continuum table in LDS and keeps the estimators there instead
    env.cellest_n_r = (e->cellest_in_lds && nc <= (e->rpkt_est_over_cont ? RPKT_CELLEST_CAP_NOCONT : RPKT_CELLEST_CAP)) ? nc : 0;
    env.cellest_n_g = (e->cellest_in_lds && nc <= GAMMA_CELLEST_CAP) ? nc : 0;
    env.scalars_in_lds = e->cellest_in_lds ? 1 : 0;
    env.estcache_on = e->estcache ? 1 : 0;
    env.ma_filters_off = e->ma_filters ? 0 : 1;
  }
  env.S = e->S;
  env.E = e->E;
  env.est_stride = 8;
  env.pair_stride = 2;
  env.P = e->P;
  env.stats = nullptr;
  env.gamma_ws = e->d_gamma_ws;
  env.bfev = e->bf_defer ? e->d_bfev : nullptr;
  env.bfev_count = e->d_bfev_count;
  env.bfev_cap = e->bfev_cap;
  env.bfrate_kept = (e->bf_defer && e->cc.ntiles == 1) ? e->d_bfrate_kept : nullptr;
  env.gamma_gi = e->d_gamma_gi;
  env.gamma_n = e->d_gamma_n;
  env.errflag = e->d_err;
  env.vpkt_queue = e->d_vpkt_queue;
  env.vpkt_count = e->d_vpkt_count;
  env.vpkt_cap = e->vpkt_cap;
#ifdef ARTIS_VISIT_COUNTS
  env.visit_counts = e->d_visit_counts;
#endif
  env.ion_absent = e->d_ion_absent;
  env.ion_popsum = e->d_ion_popsum;
  env.ma_absent_counts = e->d_absent_counts;
  env.ma_absent_eps = e->cfg.ma_absent_eps;
  return env;
}

void sort_scratch_free(SortScratch &S) {
  if (S.base) (void)hipFree(S.base);
  S = SortScratch{};
}
int sort_scratch_alloc(SortScratch &S, int64_t n) {
  sort_scratch_free(S);
  const size_t cap = (size_t)(n > 0 ? n : 1);
  const size_t matlen = (size_t)SORT_HI_MAX * ((cap + SORT_TILE - 1) / SORT_TILE);
  auto padded = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
  const size_t b_pairs = padded(sizeof(int2) * cap), b_mat = padded(sizeof(int32_t) * matlen), b_tiles = padded(sizeof(int32_t) * (matlen / SCAN_TILE + 2)),
               b_seg = padded(sizeof(int32_t) * (SORT_HI_MAX + 1));
  HIP_TRY(hipMalloc(&S.base, b_pairs + b_mat + b_tiles + 2 * b_seg));
  char *q = (char *)S.base;
  S.pairs = (int2 *)q;
  S.mat = (int32_t *)(q += b_pairs);
  S.tiles = (int32_t *)(q += b_mat);
  S.seg = (int32_t *)(q += b_tiles);
  S.chunk_base = (int32_t *)(q += b_seg);
  S.capacity = (int64_t)cap;
  return ARTIS_OK;
}
std::string sort_too_many_keys_text(int64_t nkeys) {
  return "the work-list sort takes at most " + std::to_string(SORT_MAX_KEYS) + " keys (cells x bins), this list has " + std::to_string(nkeys) +
         ": run without sorted lists (ARTIS_AMD_SORT=0)";
}
// the many-keys sort (the kernels' comment): list[0..n) by keys[] (each in [0, nkeys)) into out[0..n); n <= S.capacity
int sort_many_keys(artis_amd_engine *e, const SortScratch &S, hipStream_t s, const int32_t *list, const int32_t *keys, int32_t n, int64_t nkeys,
                   int32_t *out) {
  if (nkeys > SORT_MAX_KEYS) {
    g_last_error = sort_too_many_keys_text(nkeys);
    return ARTIS_ERR_UNSUPPORTED;
  }
  if (n <= 0 || n > S.capacity) {
    g_last_error = "sort: the list does not fit the sort's buffers";
    return ARTIS_ERR_ARG;
  }
  int keybits = 0;
  while (((int64_t)1 << keybits) < nkeys) keybits++;
  const int lobits = std::max(0, keybits - SORT_HI_BITS);
  const int nb = (int)((nkeys - 1) >> lobits) + 1;
  const int32_t ntiles = (int32_t)(((int64_t)n + SORT_TILE - 1) / SORT_TILE);
  const int32_t matlen = nb * ntiles;
  const int nscan = (matlen + SCAN_TILE - 1) / SCAN_TILE;
  const size_t lds = sizeof(int32_t) * 2 * ((size_t)1 << lobits);
  if (lds > 32 * 1024 && !e->sort_attr_set) {
    HIP_TRY(hipFuncSetAttribute((const void *)k_sort_segments, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(int32_t) * 2 << SORT_LO_BITS_MAX)));
    e->sort_attr_set = true;
  }
  hipLaunchKernelGGL(k_sort_tilehist, dim3(ntiles), dim3(SORT_TB), 0, s, keys, n, lobits, nb, ntiles, S.mat);
  hipLaunchKernelGGL(k_scan_tiles, dim3(nscan), dim3(1024), 0, s, S.mat, matlen, S.tiles);
  if (nscan > 1) {
    hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, s, S.tiles, nscan);
    hipLaunchKernelGGL(k_scan_add, dim3(nscan), dim3(1024), 0, s, S.mat, matlen, S.tiles);
  }
  hipLaunchKernelGGL(k_sort_tilescatter, dim3(ntiles), dim3(SORT_TB), 0, s, list, keys, n, lobits, nb, ntiles, S.mat, S.pairs);
  hipLaunchKernelGGL(k_sort_plan, dim3(1), dim3(1024), 0, s, S.mat, ntiles, nb, n, S.seg, S.chunk_base);
  hipLaunchKernelGGL(k_sort_segments, dim3(n / SORT_SEG_CAP + nb), dim3(BLOCK), lds, s, S.pairs, lobits, nb, S.seg, S.chunk_base, out);
  return ARTIS_OK;
}
// counting sort of list[0..n) by keys[] into out[0..n): in LDS-sized histograms for few keys, the two-pass sort for many
int sort_list(artis_amd_engine *e, hipStream_t s, const int32_t *list, const int32_t *keys, int32_t n, int64_t nkeys, int32_t *out) {
  if (nkeys > SORT_LDS_KEYS) return sort_many_keys(e, e->sort_scratch, s, list, keys, n, nkeys, out);
  const int32_t nk = (int32_t)nkeys;
  HIP_TRY(hipMemsetAsync(e->d_hist, 0, sizeof(int32_t) * (size_t)(nk + 1), s));
  hipLaunchKernelGGL(k_sort_hist_lds, dim3(sort_lds_grid(n)), dim3(BLOCK), 0, s, keys, n, e->d_hist, nk);
  const int ntiles = (nk + SCAN_TILE - 1) / SCAN_TILE;
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(1024), 0, s, e->d_hist, nk, e->d_tiles);
  hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, s, e->d_tiles, ntiles);
  hipLaunchKernelGGL(k_scan_add, dim3(ntiles), dim3(1024), 0, s, e->d_hist, nk, e->d_tiles);
  hipLaunchKernelGGL(k_sort_scatter_lds, dim3(sort_lds_grid(n)), dim3(BLOCK), 0, s, list, keys, n, e->d_hist, out, nk);
  return ARTIS_OK;
}

void free_packet_buffers(artis_amd_engine *e) {
  void **singles[] = {&e->d_pkt, &e->d_pkt_snapshot, (void **)&e->d_sorted, (void **)&e->d_perm, (void **)&e->d_gamma_ws,
                      (void **)&e->d_late_ring[0], (void **)&e->d_late_ring[1], (void **)&e->d_late_ring[2],
                      (void **)&e->d_gamma_gi, (void **)&e->d_gamma_n, (void **)&e->d_bfev, (void **)&e->d_bfev_count,
                      (void **)&e->d_vpkt_queue, (void **)&e->d_vpkt_count};
  e->bfev_cap = 0;
  e->vpkt_cap = 0;
  sort_scratch_free(e->sort_scratch);
  for (void **q : singles) {
    if (*q) (void)hipFree(*q);
    *q = nullptr;
  }
  for (int kind = 0; kind < NEXT_NKINDS; kind++)
    for (int k = 0; k < 2; k++) {
      if (e->d_lists[kind][k]) (void)hipFree(e->d_lists[kind][k]);
      if (e->d_keys[kind][k]) (void)hipFree(e->d_keys[kind][k]);
      e->d_lists[kind][k] = nullptr;
      e->d_keys[kind][k] = nullptr;
    }
  e->npackets = -1;  // nothing resident
  e->use_perm = false;
}

// k_late may take the end of this engine's populations: a build with the kernel, k_tail allowed (no virtual packets, no deferred bound-free
// events), the whole cache resident, no cold levels, and tables that fit the LDS
bool late_possible(const artis_amd_engine *e) {
  return ARTIS_LATE_KERNEL && e->late_max > 0 && e->tail_max > 0 && e->cc.ntiles == 1 && e->Mh.ncold == 0 && e->Mh.nlevels > 0 && e->Mh.nlevels < 32768 &&
         e->Mh.nalltrans > 0 && e->Mh.nbfcontinua > 0 && late_lds_bytes(e->Mh.nlevels, e->Mh.nalltrans, e->Mh.nbfcontinua) <= 160 * 1024 - 1024;
}
int ensure_packet_buffers(artis_amd_engine *e, int64_t n) {
  if (n == e->npackets && e->d_pkt) return ARTIS_OK;
  free_packet_buffers(e);
  e->pkt_bytes = pkt_store_bytes(n);
  HIP_TRY(hipMalloc(&e->d_pkt, e->pkt_bytes));
  e->P = carve_pkt_store(e->d_pkt, n);
  const size_t listbytes = sizeof(int32_t) * (size_t)(n > 0 ? n : 1);
  for (int kind = 1; kind < NEXT_NKINDS; kind++)
    for (int k = 0; k < 2; k++) {
      HIP_TRY(hipMalloc((void **)&e->d_lists[kind][k], listbytes));
      HIP_TRY(hipMalloc((void **)&e->d_keys[kind][k], listbytes));
    }
  HIP_TRY(hipMalloc((void **)&e->d_sorted, listbytes));
  HIP_TRY(hipMalloc((void **)&e->d_perm, listbytes));
  if (late_possible(e)) {  // (120 MB at 1e7 packets: only for an engine that can launch k_late)
    for (int k = 0; k < LATE_NQ; k++) HIP_TRY(hipMalloc((void **)&e->d_late_ring[k], listbytes));
  }
  if (const int rc = sort_scratch_alloc(e->sort_scratch, n)) return rc;
  e->ws_capacity = n > 0 ? n : 1;
  const size_t wsbytes = sizeof(double) * (size_t)(e->Mh.nbfcontinua_ground + 1) * (size_t)e->ws_capacity;
  HIP_TRY(hipMalloc((void **)&e->d_gamma_ws, wsbytes));
  HIP_TRY(hipMalloc((void **)&e->d_gamma_gi, wsbytes / 2));
  HIP_TRY(hipMalloc((void **)&e->d_gamma_n, sizeof(int32_t) * (size_t)e->ws_capacity));
  HIP_TRY(hipMemset(e->d_gamma_n, 0, sizeof(int32_t) * (size_t)e->ws_capacity));
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
  if (e->Mh.nbfcontinua > 0) {  // one k_rpkt launch records at most budget_r updates per packet on its list
    const int64_t cap = std::min<int64_t>((int64_t)(n > 0 ? n : 1) * e->budget_r, 0x7FFFFFF0LL);
    HIP_TRY(hipMalloc((void **)&e->d_bfev, sizeof(BfEvent) * (size_t)cap));
    HIP_TRY(hipMalloc((void **)&e->d_bfev_count, sizeof(int32_t)));
    HIP_TRY(hipMemset(e->d_bfev_count, 0, sizeof(int32_t)));
    e->bfev_cap = (int32_t)cap;
  }
#endif
#if ARTIS_OPT_VPKT_ON
  {
    const int64_t cap = std::min<int64_t>((int64_t)(n > 0 ? n : 1) * std::max(e->budget_r, 1), 0x7FFFFFF0LL);
    HIP_TRY(hipMalloc((void **)&e->d_vpkt_queue, sizeof(VpktSeed) * (size_t)cap));
    HIP_TRY(hipMalloc((void **)&e->d_vpkt_count, sizeof(int32_t)));
    HIP_TRY(hipMemset(e->d_vpkt_count, 0, sizeof(int32_t)));
    e->vpkt_cap = (int32_t)cap;
  }
#endif
  e->npackets = n;  // committed only now: a failed allocation above leaves "nothing resident" (npackets == -1)
  return ARTIS_OK;
}

int ensure_aos(artis_amd_engine *e, int64_t n) {
  if (n <= e->aos_capacity && e->d_aos) return ARTIS_OK;
  if (e->d_aos) (void)hipFree(e->d_aos);
  e->d_aos = nullptr;
  e->aos_valid = false;
  HIP_TRY(hipMalloc((void **)&e->d_aos, sizeof(artis_packet) * (size_t)(n > 0 ? n : 1)));
  e->aos_capacity = n;
  return ARTIS_OK;
}

// The npackets structs in d_aos become the resident population (buffers made by ensure_packet_buffers / ensure_aos): slots in the order of
// the packets' cells, records from the structs. What artis_amd_packets_upload does after its copy, and artis_amd_packet_init after its kernels.
int install_resident_aos(artis_amd_engine *e, int64_t npackets) {
  // a snapshot belongs to the population (and slot permutation) it was taken of
  if (e->d_pkt_snapshot) (void)hipFree(e->d_pkt_snapshot);
  e->d_pkt_snapshot = nullptr;
  if (npackets > 0) {
    e->aos_valid = true;
    e->use_perm = false;
    if (e->slot_order_by_cell && e->sort_lists && npackets >= 2 * BLOCK) {
      // counting sort of the packet indices by propagation cell (the work-list sort kernels; the lists are free now)
      int32_t *ident = e->d_lists[NEXT_RPKT][0], *keys = e->d_lists[NEXT_RPKT][1];
      const int32_t n32 = (int32_t)npackets;
      const int32_t nkeys = e->Mh.ngrid;
      hipStream_t s = nullptr;
      hipLaunchKernelGGL(k_aos_cellkeys, dim3(nblocks(npackets)), dim3(BLOCK), 0, s, e->d_aos, npackets, nkeys, ident, keys);
      if (const int rc2 = sort_list(e, s, ident, keys, n32, nkeys, e->d_perm)) return rc2;
      e->use_perm = true;
    }
    hipLaunchKernelGGL(k_aos_to_rec, dim3(nblocks(npackets)), dim3(BLOCK), 0, nullptr, e->d_aos, e->P, e->use_perm ? e->d_perm : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  return ARTIS_OK;
}

}  // namespace

namespace {
int engine_fill(artis_amd_engine *e, const artis_model *model);

// ---- sizing: the layout decisions of an engine, as pure functions of the model, the resolved configuration (engine_config.h) and the free device
// memory. engine_fill() builds what they say; artis_amd_engine_plan() reports it without building anything.

// bytes of one cell's cache row
size_t cache_row_bytes(const DevModel &h) {
  size_t per_cell = 0;
#define SZ(f, T, per) per_cell += sizeof(T) * (size_t)(per);
  ARTIS_CACHE_ARRAYS(SZ, h)
#undef SZ
  return per_cell;
}

// Macro-atom record tiers (tables.h "ON-DEMAND RECORDS"): every level a static record while the whole cell cache fits one tile; when it
// does not (even without line_dpop), static records for the lowest share of every ion's levels and a pool of ma_pool_fraction (0.15) of the rest for
// the cold levels packets reach. A given hot share (artis_amd_config.ma_hot_fraction, ARTIS_AMD_MA_HOTFRAC) is taken as it is; free_b is read only without one.
// (pool share: 0.25 in round 5. Measured on the 4e5-line set, 50^3 / 1e7, round 6 -- artis_amd_last_pool_usage(): a step leaves 48 % of a quarter-share
// pool in use; with 0.15 the tier search affords hot 0.25 instead of 0.15 and the step takes 15.9 s instead of 16.6 (pool 64 % used); with 0.10 hot 0.30,
// 15.7 s, 87 % used -- too close to a pool that is used up and emptied. profiles/r06/pool_share.txt)
void choose_record_tiers(const artis_model &model, ModelOwned &own, const EngineConfig &cfg, double free_b, DevModel *Mh, double *hotfrac) {
  const double hot = cfg.hot_given ? cfg.ma_hot : 1., pool = cfg.ma_pool;
  *Mh = make_host_model_view(model, own, hot, pool);
  *hotfrac = hot;
  if (cfg.hot_given) return;
  auto tiles_needed = [&]() -> int64_t {
    size_t per_cell = cache_row_bytes(*Mh);
    per_cell -= sizeof(double) * (size_t)Mh->ndpop;  // (dropped first when the cache does not fit: plan_cache_rows)
    const int64_t fit = std::max<int64_t>(1, (int64_t)(cache_budget_bytes(cfg, free_b) / (double)(per_cell > 0 ? per_cell : 1)));
    return (model.npts_nonempty + fit - 1) / fit;
  };
  // The largest hot share that lets the whole cache be resident (the fewer cold levels, the fewer first visits pay a fill). If none does, the
  // cache is tiled, and the share is the largest one that needs the FEWEST tiles: smaller rows, more cells resident at a time (round 6; the headline
  // forced to a quarter of its cache: 1875 ms with four tiles of static rows, 1532 ms with two tiles of rows with a quarter of the levels hot --
  // profiles/r06/tiling.md. Round 5 kept the rows static in that case: every refill of a tile emptied the pool then, and a tiled run on on-demand
  // records paid its fills again and again, 3.7 s against 3.0 s; now a fill leaves the pool and the rows of the cells that stay alone.)
  // (round 6: in steps of 0.05 below one half -- with the round-5 steps 0.5 / 0.3 / 0.2 / 0.1 a record that grew by a quarter, the fine bytes, sent
  // the 4e5-line set from 0.2 to 0.1 and doubled its fills)
  // (the fewest tiles among the shares >= 0.2: a tile saved by going lower costs more in cold levels filled on demand than the tile did -- at 11600 MB
  // two tiles at hot 0.10 take 1750 ms, three at 0.5 1620; a cache that fits ONE tile at a lower share takes that: one tile beats any tiling)
  int64_t best_nt = tiles_needed(), tiled_nt = best_nt;
  double best_h = 1., cur_h = 1., tiled_h = 1.;
  for (const double h : {0.9, 0.8, 0.7, 0.6, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25, 0.2, 0.15, 0.1, 0.05}) {
    if (best_nt <= 1) break;
    *Mh = make_host_model_view(model, own, h, pool);
    cur_h = h;
    const int64_t nt = tiles_needed();
    if (nt < best_nt) {
      best_nt = nt;
      best_h = h;
    }
    if (h > 0.199 && nt < tiled_nt) {
      tiled_nt = nt;
      tiled_h = h;
    }
  }
  if (best_nt > 1) best_h = tiled_h;
  if (cur_h != best_h) *Mh = make_host_model_view(model, own, best_h, pool);
  *hotfrac = best_h;
}

// The rows of the cell cache: all cells if that fits the budget, else one tile of cells at a time. free_b: the free device memory once the model's
// tables are resident (read by the automatic budget only).
struct CacheLayout {
  double budget = 0.;      // [B] what the rows may take
  size_t per_cell = 0;     // [B] one row
  int64_t tile_cells = 1;  // rows
  int ntiles = 1;
  bool drop_dpop = false;  // the rows are without line_dpop (the caller sets ndpop = 0)
};
int plan_cache_rows(const DevModel &h, const EngineConfig &cfg, double free_b, CacheLayout *L) {
  const int64_t ncell_all = h.npts_nonempty;
  size_t per_cell = cache_row_bytes(h);
  const double budget = cache_budget_bytes(cfg, free_b);
  {
    // The rows of line_dpop (8 bytes per line and cell: 0.9 of the 3.2 MB of a row with 110 860 lines) are dropped when the cell
    // cache does not fit one tile with them and needs fewer tiles without: the line walk then forms a line's population factor from
    // its record and the two level populations (physics.h line_dpop_at: the same expression, the same bits; two more reads per
    // line visited). artis_amd_config.keep_line_dpop (ARTIS_AMD_DPOP) = 0 / 1 forces either.
    const size_t per_without = per_cell - (sizeof(double) * (size_t)h.ndpop);
    auto tiles_of = [&](size_t per) {
      const int64_t fit = std::max<int64_t>(1, (int64_t)(budget / (double)(per > 0 ? per : 1)));
      return (ncell_all + fit - 1) / fit;
    };
    bool drop = tiles_of(per_cell) > 1 && tiles_of(per_without) < tiles_of(per_cell);
    if (cfg.keep_line_dpop >= 0) drop = cfg.keep_line_dpop == 0;
    if (cfg.dpop_strict && h.ndpop > 0 && (double)per_cell > budget) {
      g_last_error = "artis_amd_config.keep_line_dpop = 1, and the cache budget (" + std::to_string((long long)budget) + " B) cannot hold a row with line_dpop (" +
                     std::to_string(per_cell) + " B; " + std::to_string(per_without) + " B without)";
      return ARTIS_ERR_ARG;
    }
    L->drop_dpop = drop && h.ndpop > 0;
    if (L->drop_dpop) per_cell = per_without;
  }
  L->budget = budget;
  L->per_cell = per_cell;
  const int64_t fit = (int64_t)(budget / (double)(per_cell > 0 ? per_cell : 1));
  if (fit < 1 && cfg.budget_given && cfg.src_budget == CONFIG_STRUCT) {  // (a budget from the variable or from the automatic rule gets one row at a time, as ever)
    g_last_error = "artis_amd_config.cache_budget_bytes (" + std::to_string((long long)budget) + ") cannot hold one row of the cell cache (" + std::to_string(per_cell) + " B)";
    return ARTIS_ERR_ARG;
  }
  L->tile_cells = std::max<int64_t>(1, std::min<int64_t>(ncell_all > 0 ? ncell_all : 1, fit));
  L->ntiles = (int)((ncell_all + L->tile_cells - 1) / L->tile_cells);
  if (L->ntiles < 1) L->ntiles = 1;
  if (ARTIS_OPT_VPKT_ON && L->ntiles > 1) {
    // a virtual packet's ray reads the cache rows of every cell up to the grid's edge (vpkt.cc:183): all of them have to be resident
    g_last_error = "this build has VPKT_ON and the cell cache does not fit one tile (" + std::to_string(per_cell) + " B per cell x " +
                   std::to_string((long long)ncell_all) + " cells): virtual packets need every cell's row resident";
    return ARTIS_ERR_UNSUPPORTED;
  }
  return ARTIS_OK;
}

// the population works through the cells in batches whose cooling terms fit its scratch (artis_amd_config.pop_scratch_bytes: ~2 GB), allocated after the
// cache rows: cells per batch, and the bytes of the scratch
int64_t pop_batch_cells(const DevModel &h, int64_t tile_cells, const EngineConfig &cfg) {
  const int64_t per = std::max<int64_t>(1, (int64_t)h.nupcum) * (int64_t)sizeof(double);
  return std::max<int64_t>(1, std::min<int64_t>(tile_cells, (int64_t)cfg.pop_scratch / per));
}
size_t pop_scratch_alloc_bytes(const DevModel &h, int64_t batch) {
  return (size_t)(batch * std::max<int64_t>(1, (int64_t)h.nupcum) * (int64_t)sizeof(double)) + 64;
}

// bytes of the model's tables on the device (what engine_fill uploads before it sizes the cache: upload_array's sizes)
int64_t model_table_bytes(const DevModel &h) {
  int64_t bytes = 0;
#define SZ(f, T, count) bytes += (int64_t)sizeof(T) * std::max<int64_t>(1, (int64_t)(count));
  ARTIS_MODEL_ARRAYS(SZ, h)
#undef SZ
#define SZO(f, T, count) \
  if (h.f) bytes += (int64_t)sizeof(T) * std::max<int64_t>(1, (int64_t)(count));
  ARTIS_MODEL_OPTIONAL_ARRAYS(SZO, h)
#undef SZO
  const int ndim = (h.gridtype == ARTIS_GRID_SPHERICAL1D) ? 1 : ((h.gridtype == ARTIS_GRID_CYLINDRICAL2D) ? 2 : 3);
  for (int a = 0; a < 3; a++) bytes += (int64_t)sizeof(double) * std::max<int64_t>(1, (a >= ndim) ? 1 : h.ncoordgrid[a]);
  bytes += (int64_t)sizeof(int32_t) * std::max<int64_t>(1, h.nphixstargets_total);  // the target -> level table
  return bytes;
}

// RCCL entry points, resolved at run time from the librccl the process already has (a host that links RCCL itself, or
// torch's own copy in bench.py) or else from the ROCm installation: the engine library itself carries no link-time
// dependency on a particular librccl, and a communicator handed in by the caller is used with the library it came from.
struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;  // optional: artis_amd_comm_count()
  bool ok = false;
};
const RcclApi &rccl_api() {
  static RcclApi api = [] {
    RcclApi a;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so"}) {
      h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
      if (h) break;
    }
    if (!h)
      for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
      }
    if (!h) return a;
    a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
    a.AllReduce = (decltype(a.AllReduce))dlsym(h, "ncclAllReduce");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
    a.CommCount = (decltype(a.CommCount))dlsym(h, "ncclCommCount");
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce && a.GetErrorString;
    return a;
  }();
  return api;
}
#define RCCL_TRY(expr)                                                                             \
  do {                                                                                             \
    ncclResult_t _r = (expr);                                                                      \
    if (_r != ncclSuccess) {                                                                       \
      g_last_error = std::string(#expr) + ": " + rccl_api().GetErrorString(_r);                    \
      return ARTIS_ERR_RCCL;                                                                       \
    }                                                                                              \
  } while (0)
}  // namespace

extern "C" {

const char *artis_amd_last_error(void) { return g_last_error.c_str(); }
int artis_amd_abi_version(void) { return 6; }
const char *artis_amd_options_preset(void) {
#if defined(ARTIS_PRESET_NAME)  // given by the build (artis_amd/build.py): the presets of the reference's CI option sets
  return ARTIS_PRESET_NAME;
#elif defined(ARTIS_PRESET_NLTENEBULAR_LINEEST)
  return "nltenebular_lineest";
#elif defined(ARTIS_PRESET_CHRISTINENONTHERMAL)
  return "christinenonthermal";
#elif defined(ARTIS_PRESET_NLTEPHOTOSPHERIC)
  return "nltephotospheric";
#elif defined(ARTIS_PRESET_NLTEWITHOUTNONTHERMAL)
  return "nltewithoutnonthermal";
#elif defined(ARTIS_PRESET_NLTENEBULAR)
  return "nltenebular";
#elif defined(ARTIS_PRESET_KILONOVA_EXPOPAC)
  return "kilonova_expopac";
#elif defined(ARTIS_PRESET_CLASSIC_EXPOPAC_THERM)
  return "classic_expopac_therm";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMA_GREY)
  return "kilonova_gamma_grey";
#elif defined(ARTIS_PRESET_CLASSIC_GAMMA_XCOM)
  return "classic_gamma_xcom";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMA_BARNES)
  return "kilonova_gamma_barnes";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMA_WOLLAEGER)
  return "kilonova_gamma_wollaeger";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMA_GUTTMAN)
  return "kilonova_gamma_guttman";
#elif defined(ARTIS_PRESET_KILONOVA_GAMMAPRODUCTS)
  return "kilonova_gammaproducts";
#elif defined(ARTIS_PRESET_KILONOVA_BARNES)
  return "kilonova_barnes";
#elif defined(ARTIS_PRESET_KILONOVA_WOLLAEGER)
  return "kilonova_wollaeger";
#elif defined(ARTIS_PRESET_KILONOVA_LTE)
  return "kilonova_lte";
#else
  return "classic";
#endif
}
size_t artis_amd_sizeof_packet(void) { return sizeof(artis_packet); }

}  // extern "C"

namespace {
// what the engine requires of a model before anything is sized or uploaded (artis_amd_engine_create_ex, artis_amd_engine_plan)
int validate_model(const artis_model *model) {
  if (model->gridtype != ARTIS_GRID_CARTESIAN3D && model->gridtype != ARTIS_GRID_SPHERICAL1D &&
      model->gridtype != ARTIS_GRID_CYLINDRICAL2D) {
    g_last_error = "unknown grid type";
    return ARTIS_ERR_UNSUPPORTED;
  }
  // the per-packet list of ground-continuum contributions (physics.h chi_bf_gammacontr) relies on the order the
  // reference builds these tables in: groundcont_nu_edge rising (input.cc:802) and, with allcont sorted by nu_edge
  // (input.cc:892), a non-decreasing nearest-edge index (input.cc:703)
  for (int i = 1; i < model->nbfcontinua_ground; i++) {
    if (model->groundcont_nu_edge[i] < model->groundcont_nu_edge[i - 1]) {
      g_last_error = "groundcont_nu_edge is not in ascending order";
      return ARTIS_ERR_ARG;
    }
  }
  for (int i = 0, last = -1; i < model->nbfcontinua; i++) {
    const int gi = model->allcont_groundcontestimindex[i];
    if (gi < 0) continue;
    if (gi < last || gi >= model->nbfcontinua_ground) {
      g_last_error = "allcont_groundcontestimindex does not rise with nu_edge";
      return ARTIS_ERR_ARG;
    }
    last = gi;
  }
  for (int i = 0; i < model->nlevels; i++) {  // what a packed macro-atom transition target can hold (tables.h MaTarget)
    if (model->level_ndowntrans[i] >= MATGT_MAX_NTRANS || model->level_nuptrans[i] >= MATGT_MAX_NTRANS) {
      g_last_error = "a level has more transitions than a packed transition target can describe";
      return ARTIS_ERR_UNSUPPORTED;
    }
  }
  // k_cooling_tail reads what the entries of an ion's cooling list after the collisional excitations are from the list itself
  // (coolinglist_type / _level / _phixstargetindex): they must be in the order calculate_cooling_rates_ion() writes them
  // (kpkt.cc:122-190: the collisional ionisations level by level and target by target, then the bound-free terms likewise)
  for (int el = 0; el < model->nelements && model->ncoolingterms > 0; el++)
    for (int ion = 0; ion < model->elem_nions[el]; ion++) {
      const int ui = model->elem_uniqueionindexstart[el] + ion;
      int k = ((model->elem_lowest_ionstage[el] + ion - 1) > 0) ? 1 : 0;
      const int start = model->ion_uniquelevelindexstart[ui];
      for (int l = 0; l < model->ion_nlevels[ui]; l++) k += (model->level_nuptrans[start + l] > 0) ? 1 : 0;
      bool ok = true;
      if (ion < model->elem_nions[el] - 1 && model->nbfcontinua > 0) {
        const int off = model->ion_coolingoffset[ui];
        for (int pass = 0; pass < 2 && ok; pass++)
          for (int l = 0; l < model->ion_nlevels_ionising[ui] && ok; l++)
            for (int t = 0; t < model->level_nphixstargets[start + l] && ok; t++, k++)
              ok = k < model->ion_ncoolingterms[ui] && model->coolinglist_type[off + k] == (pass == 0 ? ARTIS_COOLING_COLLION : ARTIS_COOLING_FREEBOUND) &&
                   model->coolinglist_level[off + k] == l && model->coolinglist_phixstargetindex[off + k] == t;
      }
      if (!ok || k != model->ion_ncoolingterms[ui]) {
        g_last_error = "the cooling list of an ion is not in the order of calculate_cooling_rates_ion()";
        return ARTIS_ERR_ARG;
      }
    }
  {
    // alltrans is laid out level by level, downward then upward transitions, without gaps (input.cc:565): k_matrans takes a block's
    // extent from its first and last segment, ma_entry_pos() an entry's place from its offset, and the records' filter lines are
    // counted from a level's first entry
    int64_t next = 0;
    for (int ul = 0; ul < model->nlevels; ul++) {
      if (model->level_alltrans_startdown[ul] != next || model->level_ndowntrans[ul] < 0 || model->level_nuptrans[ul] < 0) {
        g_last_error = "alltrans is not contiguous in level order (level_alltrans_startdown[i+1] == startdown[i] + ndown[i] + nup[i])";
        return ARTIS_ERR_ARG;
      }
      next += (int64_t)model->level_ndowntrans[ul] + model->level_nuptrans[ul];
    }
    if (next != model->nalltrans) {
      g_last_error = "the last level's transitions do not end at nalltrans";
      return ARTIS_ERR_ARG;
    }
  }
  for (int i = 0; i < model->nions; i++) {  // DevModel::alltrans_tlevel16: a target level within its ion in 16 bits
    if (model->ion_nlevels[i] > 65535) {
      g_last_error = "an ion has more levels than a 16-bit target level can describe";
      return ARTIS_ERR_UNSUPPORTED;
    }
  }
  {  // the r-packet list's keys (cells x frequency bins) have to fit the work-list sort, unless the lists stay unsorted
    const char *b = std::getenv("ARTIS_AMD_SORT");
    const int64_t nkeys = (int64_t)model->ngrid * SORT_NUBINS;
    if (nkeys > SORT_MAX_KEYS && !(b && std::atoi(b) == 0)) {
      g_last_error = sort_too_many_keys_text(nkeys);
      return ARTIS_ERR_UNSUPPORTED;
    }
  }
  return ARTIS_OK;
}
}  // namespace

extern "C" {

size_t artis_amd_sizeof_config(void) { return sizeof(artis_amd_config); }
size_t artis_amd_sizeof_plan(void) { return sizeof(artis_amd_plan); }
void artis_amd_config_default(artis_amd_config *cfg) {
  if (cfg) config_set_default(cfg);
}

int artis_amd_engine_create(const artis_model *model, int device, artis_amd_engine **out) {
  return artis_amd_engine_create_ex(model, device, nullptr, out);
}

int artis_amd_engine_create_ex(const artis_model *model, int device, const artis_amd_config *cfg, artis_amd_engine **out) {
  if (out) *out = nullptr;
  if (!model || !out) {
    g_last_error = "null argument";
    return ARTIS_ERR_ARG;
  }
  artis_amd_config checked;  // the configuration first: a caller's mistake is reported before the device is touched
  if (const int rc = config_copy_checked(cfg, &checked, &g_last_error)) return rc;
  if (const int rc = validate_model(model)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_last_error = "no HIP device: the artis_amd engine has no CPU path";
    return ARTIS_ERR_NODEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  artis_amd_engine *e = new artis_amd_engine();
  e->device = device;
  apply_config(e, checked);
  const int rc = engine_fill(e, model);
  if (rc != ARTIS_OK) {  // release whatever was allocated before the failing call (g_last_error is already set)
    artis_amd_engine_destroy(e);
    return rc;
  }
  *out = e;
  return ARTIS_OK;
}

}  // extern "C"

namespace {
int engine_fill(artis_amd_engine *e, const artis_model *model) {
  const int device = e->device;
  {  // macro-atom record tiers (choose_record_tiers): given, or chosen from the cache budget -- then from what is free on the device now
    double free_b = 0.;
    if (!e->cfg.hot_given) {
      size_t f = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&f, &total_b));
      free_b = (double)f;
    }
    choose_record_tiers(*model, e->own, e->cfg, free_b, &e->Mh, &e->ma_hotfrac);
  }
  e->model_copy = *model;
  e->own_matransblock_start.assign(model->level_matransblock_start, model->level_matransblock_start + model->nlevels);
  e->model_copy.level_matransblock_start = e->own_matransblock_start.data();
  e->M = e->Mh;
  const DevModel &h = e->Mh;
#define UP(f, T, count)                                                                     \
  {                                                                                         \
    int rc = upload_array<T>(e->model_allocs, h.f, (int64_t)(count), (const T **)&e->M.f);  \
    if (rc != ARTIS_OK) return rc;                                                          \
  }
  ARTIS_MODEL_ARRAYS(UP, h)
#undef UP
#define UPMO(f, T, count)                                                                     \
  {                                                                                           \
    e->M.f = nullptr;                                                                         \
    if (h.f) {                                                                                \
      int rc = upload_array<T>(e->model_allocs, h.f, (int64_t)(count), (const T **)&e->M.f);  \
      if (rc != ARTIS_OK) return rc;                                                          \
    }                                                                                         \
  }
  ARTIS_MODEL_OPTIONAL_ARRAYS(UPMO, h)
#undef UPMO
  if ((ARTIS_OPT_GAMMA_THERMALISATION_SCHEME == ARTIS_GAMMA_WOLLAEGER || ARTIS_OPT_GAMMA_THERMALISATION_SCHEME == ARTIS_GAMMA_GUTTMAN) &&
      !e->M.rho_tmin) {
    g_last_error = "this build integrates gamma-ray column densities: artis_model.rho_tmin is required";
    return ARTIS_ERR_ARG;
  }
  if ((ARTIS_OPT_GAMMA_THERMALISATION_SCHEME == ARTIS_GAMMA_BARNES || ARTIS_OPT_PARTICLE_THERMALISATION_SCHEME == ARTIS_PARTICLE_BARNES) &&
      !(h.mtot_input > 0. && h.ejecta_kinetic_energy > 0.)) {
    g_last_error = "this build uses a Barnes thermalisation efficiency: artis_model.mtot_input and ejecta_kinetic_energy are required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_USE_XCOM_GAMMAPHOTOION && (!e->M.xcom_elem_start || !e->M.xcom_energy || !e->M.xcom_sigma || !e->M.elem_meannucmass)) {
    g_last_error = "this build has USE_XCOM_GAMMAPHOTOION: artis_model.xcom_elem_start / xcom_energy / xcom_sigma and elem_meannucmass are required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_DETAILED_LINE_ESTIMATORS_ON && (!e->M.detailed_lineindices || h.detailed_linecount <= 0)) {
    g_last_error = "this build has DETAILED_LINE_ESTIMATORS_ON: artis_model.detailed_lineindices / detailed_linecount are required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_BFEST_SUBSET && !e->M.allcont_bfestimindex) {
    g_last_error = "this build keeps bound-free estimators for a subset of the continua: artis_model.allcont_bfestimindex / nbfestim are required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_NT_ON && (!e->M.elem_meannucmass || !e->M.ion_nt_sum_q_over_binding)) {
    g_last_error = "this build has NT_ON: artis_model.elem_meannucmass and ion_nt_sum_q_over_binding are required";
    return ARTIS_ERR_ARG;
  }
  for (int a = 0; a < 3; a++) {
    const int ndim = (h.gridtype == ARTIS_GRID_SPHERICAL1D) ? 1 : ((h.gridtype == ARTIS_GRID_CYLINDRICAL2D) ? 2 : 3);  // get_ndim grid.cc:120
    const int64_t cnt = (a >= ndim) ? 1 : h.ncoordgrid[a];
    int rc = upload_array<double>(e->model_allocs, h.coord_pos_min_tmin[a], cnt, &e->M.coord_pos_min_tmin[a]);
    if (rc != ARTIS_OK) return rc;
  }
  // allphixstarget index -> level
  {
    std::vector<int32_t> tl((size_t)(h.nphixstargets_total > 0 ? h.nphixstargets_total : 1), 0);
    for (int ul = 0; ul < h.nlevels; ul++)
      for (int t = 0; t < h.level_nphixstargets[ul]; t++) tl[h.level_phixstargetstart[ul] + t] = ul;
    const int32_t *d = nullptr;
    int rc = upload_array<int32_t>(e->model_allocs, tl.data(), h.nphixstargets_total, &d);
    if (rc != ARTIS_OK) return rc;
    e->d_target_level = (int32_t *)d;
  }
  // per-cell cache: all cells if that fits the budget, else one tile of cells at a time (plan_cache_rows)
  const int64_t ncell_all = h.npts_nonempty;
  {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    CacheLayout L;
    if (const int rc = plan_cache_rows(h, e->cfg, (double)free_b, &L)) return rc;
    if (L.drop_dpop) {
      e->Mh.ndpop = 0;
      e->M.ndpop = 0;
    }
    e->cache_budget = L.budget;
    e->cc.cache_bytes_per_cell = L.per_cell;
    e->cc.res.tile_cells = L.tile_cells;
    e->cc.ntiles = L.ntiles;
    e->cc.tile_lo = 0;
    e->cc.tile_hi = (int)std::min<int64_t>(ncell_all, e->cc.res.tile_cells);
  }
  const int64_t nrows = e->cc.res.tile_cells;  // rows allocated
#define CA(f, T, per)                                                                       \
  {                                                                                         \
    T *d = nullptr;                                                                         \
    HIP_TRY(hipMalloc((void **)&d, sizeof(T) * (size_t)(nrows * (int64_t)(per) + MAREC_SLACK)));    \
    e->cache_allocs.push_back(d);                                                           \
    e->K.f = d;                                                                             \
  }
  ARTIS_CACHE_ARRAYS(CA, h)
#undef CA
  // estimators: one contiguous block [cell][8]{J, nuJ, ff, col, dep_gamma, dep_electron, dep_positron, dep_alpha} | [cell][ground continuum][2]{gamma, bfheat} | scalars
  const int64_t ncell = ncell_all;  // estimators cover every cell
  const int64_t g = h.nbfcontinua_ground > 0 ? h.nbfcontinua_ground : 1;
  // ... | scalars | ([cell][bin][2]{radfieldbin_J, radfieldbin_nuJ}) | (bfrate_raw)]
  const int64_t nbinest = ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON ? ncell * ARTIS_OPT_RADFIELDBINCOUNT : 0;
  const int64_t nbfest = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? ncell * (int64_t)h.nbfestim : 0;
  const int64_t nlineest = ARTIS_OPT_DETAILED_LINE_ESTIMATORS_ON ? ncell * (int64_t)h.detailed_linecount : 0;
  // ... | (vspecpol | vgrid_flux)]: the observers' spectra of a VPKT_ON build, inside the block the all-reduce covers
  int64_t nvspec = 0, nvgrid = 0;
#if ARTIS_OPT_VPKT_ON
  {
    VpktConfig V;
    if (!make_vpkt_config(*model, V)) {
      g_last_error = "this build has VPKT_ON: artis_model.vpkt_* (the configuration read from vpkt.txt) is required";
      return ARTIS_ERR_ARG;
    }
    HIP_TRY(hipMalloc((void **)&e->d_vpkt_config, sizeof(VpktConfig)));
    e->model_allocs.push_back(e->d_vpkt_config);
    HIP_TRY(hipMemcpy(e->d_vpkt_config, &V, sizeof(V), hipMemcpyHostToDevice));
    e->M.vpkt = e->d_vpkt_config;
    nvspec = (int64_t)ARTIS_VSPEC_TIMEBINS * V.nobsdirections * V.nspectraperobsdir * ARTIS_VSPEC_NUBINS * 3;
    nvgrid = V.vgrid_on ? (int64_t)ARTIS_VGRID_NY * ARTIS_VGRID_NZ * V.grid_nwavelengthranges * V.nobsdirections * 3 : 0;
    e->tail_max = 0;  // k_tail takes a packet through any number of steps in one launch: more events than the queue is sized for
  }
#endif
  e->nvspec = nvspec;
  e->nvgrid = nvgrid;
  e->est_ndoubles = ncell * 8 + 2 * ncell * g + ARTIS_NSCALARS + 2 * nbinest + nbfest + 2 * nlineest + nvspec + nvgrid;
  HIP_TRY(hipMalloc((void **)&e->d_est, sizeof(double) * (size_t)e->est_ndoubles));
  HIP_TRY(hipMemset(e->d_est, 0, sizeof(double) * (size_t)e->est_ndoubles));
  // [cell][8] {J, nuJ, ffheating, colheating, dep_gamma, dep_electron, dep_positron, dep_alpha}: one 64-byte record per cell
  // (physics.h Env::est_stride), then [cell][ground continuum][2] {gamma, bfheating}
  e->E.J = e->d_est;
  e->E.nuJ = e->d_est + 1;
  e->E.ffheatingestimator = e->d_est + 2;
  e->E.colheatingestimator = e->d_est + 3;
  e->E.dep_estimator_gamma = e->d_est + 4;
  e->E.dep_estimator_electron = e->d_est + 5;
  e->E.dep_estimator_positron = e->d_est + 6;
  e->E.dep_estimator_alpha = e->d_est + 7;
  e->E.gammaestimator = e->d_est + 8 * ncell;
  e->E.bfheatingestimator = e->d_est + 8 * ncell + 1;
  e->E.scalars = e->d_est + 8 * ncell + 2 * ncell * g;
  e->E.radfieldbin_J = nbinest ? e->E.scalars + ARTIS_NSCALARS : nullptr;
  e->E.radfieldbin_nuJ = nbinest ? e->E.radfieldbin_J + 1 : nullptr;  // [cell][bin][2] {J, nuJ}
  e->E.bfrate_raw = nbfest ? e->E.scalars + ARTIS_NSCALARS + 2 * nbinest : nullptr;
  e->E.Jb_lu_raw = nlineest ? e->E.scalars + ARTIS_NSCALARS + 2 * nbinest + nbfest : nullptr;
  e->E.Jb_lu_contribcount = nlineest ? e->E.Jb_lu_raw + nlineest : nullptr;
  e->E.vspecpol = nvspec ? e->E.scalars + ARTIS_NSCALARS + 2 * nbinest + nbfest + 2 * nlineest : nullptr;
  e->E.vgrid_flux = nvgrid ? e->E.vspecpol + nvspec : nullptr;
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
  if (nbfest > 0 && h.nbfcontinua > 0 && e->cc.ntiles == 1) {
    const size_t bytes = sizeof(double) * (size_t)ncell * (size_t)h.nbfcontinua;
    HIP_TRY(hipMalloc((void **)&e->d_bfrate_kept, bytes));
    HIP_TRY(hipMemset(e->d_bfrate_kept, 0, bytes));
  }
#endif
  HIP_TRY(hipMalloc((void **)&e->d_stats, sizeof(unsigned long long) * ARTIS_NSTATS));
  HIP_TRY(hipMemset(e->d_stats, 0, sizeof(unsigned long long) * ARTIS_NSTATS));
  HIP_TRY(hipMalloc((void **)&e->d_count, sizeof(int32_t) * (2 * NEXT_NKINDS + 2)));
  HIP_TRY(hipMemset(e->d_count, 0, sizeof(int32_t) * (2 * NEXT_NKINDS + 2)));
  e->d_err = e->d_count + (2 * NEXT_NKINDS);
  e->d_late_bail = e->d_err + 1;  // (k_late's count of waves that gave up waiting: travels with the counters)
  HIP_TRY(hipHostMalloc((void **)&e->h_counts, sizeof(int32_t) * (2 * NEXT_NKINDS + 2), hipHostMallocDefault));
  HIP_TRY(hipMalloc((void **)&e->d_cursors, sizeof(int32_t) * PULL_SLOTS));  // (work_pull.h: the chunk cursors + the launch's "list used up" flag)
  HIP_TRY(hipMalloc((void **)&e->cc.d_fill_cells, sizeof(int32_t) * (size_t)(ncell_all > 0 ? ncell_all : 1)));
  if (e->cc.ntiles > 1) {  // rows for a set of cells at a time: the table of rows, no cell resident yet
    HIP_TRY(hipMalloc((void **)&e->cc.d_krow, sizeof(int32_t) * (size_t)ncell_all));
    e->cc.res.init(ncell_all);
    HIP_TRY(hipMemset(e->cc.d_krow, 0xFF, sizeof(int32_t) * (size_t)ncell_all));
    e->cc.h_cell_grid.assign((size_t)ncell_all, 0);
    for (int g = 0; g < h.ngrid; g++)
      if (h.propcell_nonemptymgi[g] >= 0) e->cc.h_cell_grid[(size_t)h.propcell_nonemptymgi[g]] = g;
  }
  {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    e->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  HIP_TRY(hipMalloc((void **)&e->d_hist, sizeof(int32_t) * (SORT_LDS_KEYS + 1)));
  HIP_TRY(hipMalloc((void **)&e->d_tiles, sizeof(int32_t) * (SORT_LDS_KEYS / SCAN_TILE + 2)));
  HIP_TRY(hipEventCreate(&e->ev0));
  HIP_TRY(hipEventCreate(&e->ev1));
  HIP_TRY(hipEventCreate(&e->ev2));
  HIP_TRY(hipEventCreate(&e->ev3));
  read_switches(e);
  {
    // the static part of every macro-atom record (tables.h: filter entries that are never counted) is written once
    const int64_t nrows_ = e->cc.res.tile_cells;  // every resident row; the static parts do not depend on the cell
    Env env0 = make_env(e);
    env0.K = e->K;
    hipLaunchKernelGGL(k_mainit, dim3(nblocks(nrows_ * e->Mh.nlevels)), dim3(BLOCK), 0, nullptr, env0, nrows_);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
  }
  {
    // the population works through the cells in batches whose cooling terms fit its scratch (pop_batch_cells)
    e->cc.pop_batch = pop_batch_cells(e->Mh, e->cc.res.tile_cells, e->cfg);
    HIP_TRY(hipMalloc((void **)&e->cc.d_collexc_terms, pop_scratch_alloc_bytes(e->Mh, e->cc.pop_batch)));
  }
  // (a build whose slow path fills records by the lane has no fill into a static slot: everything is populated)
  // (... and a model with cold levels keeps the full population of its static records unless ARTIS_AMD_MA_ABSENT_EPS asks: its step was measured
  // slower with the skip, profiles/r12/absent_ions.md)
  if (e->Mh.ncold > 0 && e->cfg.src_absent == CONFIG_DEFAULT) e->cfg.ma_absent_eps = -1.;
  if (e->cfg.ma_absent_eps >= 0. && ARTIS_MA_WAVE_FILL && e->Mh.nions > 0 && e->Mh.nalltrans > 0) {
    const size_t nb = (size_t)e->cc.res.tile_cells * (size_t)e->Mh.nions;
    HIP_TRY(hipMalloc((void **)&e->d_ion_absent, nb));
    HIP_TRY(hipMemset(e->d_ion_absent, 0, nb));
    HIP_TRY(hipMalloc((void **)&e->d_ion_popsum, nb * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&e->d_absent_counts, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(e->d_absent_counts, 0, 2 * sizeof(unsigned long long)));
  }
  if (e->trace) trace_config(e);
  if (e->trace)
    fprintf(stderr, "[artis_amd] record tiers: static records for %.2f of every ion's levels, %d cold levels, pool of %d slots per resident cell; %d tile(s) of %lld cells, %zu B per cell\n",
            e->ma_hotfrac, e->Mh.ncold, e->Mh.ma_pool_slots, e->cc.ntiles, (long long)e->cc.res.tile_cells, e->cc.cache_bytes_per_cell);
  return ARTIS_OK;
}
}  // namespace

extern "C" {

void artis_amd_engine_destroy(artis_amd_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->comm && rccl_api().ok) (void)rccl_api().CommDestroy(e->comm);
  free_all(e->model_allocs);
  free_all(e->cell_allocs);
  free_all(e->cache_allocs);
  free_packet_buffers(e);
  spec_free(e->spec);
  rf_free(e->rf);
  ib_free(e->ib);
  decay_free(e->decay);
  dep_free(e->dep);
  pinit_free(e->pinit);
  tb_free(e->tb);
  bfh_free(e->bfh);
  rc_free(e->rc);
  pi_free(e->pi);
  if (e->h_counts) (void)hipHostFree(e->h_counts);
  void *ptrs[] = {e->d_est, e->d_stats, e->d_aos, e->d_hist, e->d_tiles, e->d_count, e->d_cursors, e->cc.d_krow, e->cc.d_fill_cells, e->cc.d_waiting,
                  e->d_bfrate_kept, e->cc.d_collexc_terms, e->d_visit_counts, e->d_ion_absent, e->d_ion_popsum, e->d_absent_counts};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  for (hipEvent_t ev : {e->ev0, e->ev1, e->ev2, e->ev3})
    if (ev) (void)hipEventDestroy(ev);
  delete e;
}

}  // extern "C"

namespace {

// artis_amd_set_cellstate in two halves, shared with artis_amd_set_cellstate_photoion (stage_photoion.h), which computes
// corrphotoioncoeff between them. The first: the uploads and what the build's options need from the host; corrphotoioncoeff_follows:
// the caller makes that array on the device before cellstate_finish.
int cellstate_upload(artis_amd_engine *e, const artis_cellstate *cells, const artis_timestep *ts, const bool corrphotoioncoeff_follows) {
  HIP_TRY(hipSetDevice(e->device));
  e->have_cells = false;  // until every array of the new state is resident
  free_all(e->cell_allocs);
  e->pi_coeff = nullptr;
  const DevModel &h = e->Mh;
  DevCells hc = make_host_cells_view(*cells);
  std::vector<float> zero_ffegrp;
  if (!hc.ffegrp) {  // no gamma packets will be handed over: the opacities of gammapkt.cc are never evaluated
    zero_ffegrp.assign((size_t)(h.npts_nonempty > 0 ? h.npts_nonempty : 1), 0.f);
    hc.ffegrp = zero_ffegrp.data();
  }
#define UPC(f, T, count)                                                                   \
  {                                                                                        \
    int rc = upload_array<T>(e->cell_allocs, hc.f, (int64_t)(count), (const T **)&e->C.f); \
    if (rc != ARTIS_OK) return rc;                                                         \
  }
  ARTIS_CELL_ARRAYS(UPC, h)
#undef UPC
#define UPO(f, T, count)                                                                     \
  {                                                                                          \
    e->C.f = nullptr;                                                                        \
    if (hc.f) {                                                                              \
      int rc = upload_array<T>(e->cell_allocs, hc.f, (int64_t)(count), (const T **)&e->C.f); \
      if (rc != ARTIS_OK) return rc;                                                         \
    }                                                                                        \
  }
  const int64_t nt_stored = (hc.nt_exc_count && hc.nt_excitations_stored > 0) ? hc.nt_excitations_stored : 0;
  ARTIS_CELL_OPTIONAL_ARRAYS(UPO, h)
#undef UPO
  e->C.nt_excitations_stored = (int32_t)nt_stored;
  e->C.nt_ionratecoeff = nullptr;
  e->C.nt_ionenrate_cum = nullptr;
  // what the options this library was built with need from the host
  if (!ARTIS_OPT_USE_LUT_PHOTOION && h.nphixstargets_total > 0 && !e->C.corrphotoioncoeff && !corrphotoioncoeff_follows) {
    g_last_error = "this build has USE_LUT_PHOTOION off: artis_cellstate.corrphotoioncoeff is required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON && (!e->C.radfieldbin_W || !e->C.radfieldbin_T_R)) {
    g_last_error = "this build has the multibin radiation field on: artis_cellstate.radfieldbin_W / _T_R are required";
    return ARTIS_ERR_ARG;
  }
  e->expopac_own = false;
  if (ARTIS_OPT_USE_CALCULATED_MEANATOMICWEIGHT && (ARTIS_OPT_USE_XCOM_GAMMAPHOTOION || ARTIS_OPT_NT_ON) && !e->C.elem_meanweight) {
    g_last_error = "this build has USE_CALCULATED_MEANATOMICWEIGHT and reads element number densities: artis_cellstate.elem_meanweight is required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_OPT_DETAILED_LINE_ESTIMATORS_ON && !e->C.Jb_lu_normed) {
    g_last_error = "this build has DETAILED_LINE_ESTIMATORS_ON: artis_cellstate.Jb_lu_normed is required";
    return ARTIS_ERR_ARG;
  }
  if (ARTIS_EXPOPAC_TABLES) {
    // the tables of calculate_expansion_opacities(): the host's, or (both NULL) made by the engine at cell-cache population
    const bool need_planck = ARTIS_OPT_RPKT_BB_THERMALISATION;
    if (!e->C.expansionopacities && !e->C.expansionopacity_planck_cumulative) {
      const size_t cnt = (size_t)(h.npts_nonempty > 0 ? h.npts_nonempty : 1) * ARTIS_EXPOPAC_NBINS;
      float *dk = nullptr;
      double *dp = nullptr;
      HIP_TRY(hipMalloc((void **)&dk, sizeof(float) * cnt));
      e->cell_allocs.push_back(dk);
      HIP_TRY(hipMemset(dk, 0, sizeof(float) * cnt));
      HIP_TRY(hipMalloc((void **)&dp, sizeof(double) * cnt));
      e->cell_allocs.push_back(dp);
      HIP_TRY(hipMemset(dp, 0, sizeof(double) * cnt));
      e->C.expansionopacities = dk;
      e->C.expansionopacity_planck_cumulative = dp;
      e->expopac_own = true;
    } else if (!e->C.expansionopacities || (need_planck && !e->C.expansionopacity_planck_cumulative)) {
      g_last_error = "expansion-opacity build: hand over both artis_cellstate.expansionopacities and (with a thermalisation "
                     "probability) .expansionopacity_planck_cumulative, or neither (the engine then calculates them)";
      return ARTIS_ERR_ARG;
    }
  }
  e->S = make_step(*ts);
  return ARTIS_OK;
}

// the second half: what is derived once per cell state, then the cell cache
int cellstate_finish(artis_amd_engine *e) {
  const DevModel &h = e->Mh;
#if ARTIS_OPT_NT_ON
  const int64_t nt_stored = e->C.nt_excitations_stored;
  if (!e->C.nt_frac_ionisation || !e->C.nt_frac_excitation || !e->C.nt_deposition_rate_density || !e->C.nt_eff_ionpot ||
      !e->C.nt_prob_num_auger || !e->C.nt_ionenfrac_num_auger || !e->C.nt_exc_count ||
      (nt_stored > 0 && (!e->C.nt_exc_frac_deposition || !e->C.nt_exc_ratecoeffperdeposition || !e->C.nt_exc_alltransindex))) {
    g_last_error = "this build has NT_ON: the Spencer-Fano solution (artis_cellstate.nt_*) is required";
    return ARTIS_ERR_ARG;
  }
  {
    const size_t bytes = sizeof(double) * (size_t)(h.npts_nonempty > 0 ? h.npts_nonempty : 1) * (size_t)h.nions;
    HIP_TRY(hipMalloc((void **)&e->C.nt_ionratecoeff, bytes));
    e->cell_allocs.push_back(e->C.nt_ionratecoeff);
    HIP_TRY(hipMalloc((void **)&e->C.nt_ionenrate_cum, bytes));
    e->cell_allocs.push_back(e->C.nt_ionenrate_cum);
    if (h.npts_nonempty > 0) {
      const Env env = make_env(e);
      hipLaunchKernelGGL(k_nt_cells, dim3((h.npts_nonempty + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, nullptr, env, h.npts_nonempty);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
      int32_t err = 0;
      HIP_TRY(hipMemcpy(&err, e->d_err, sizeof(err), hipMemcpyDeviceToHost));
      if (err != 0) {
        (void)hipMemset(e->d_err, 0, sizeof(int32_t));
        g_last_error = "the Spencer-Fano solution is inconsistent (Auger probabilities do not sum to one): error flag " + std::to_string(err);
        return ARTIS_ERR_ARG;
      }
    }
  }
#endif
  e->have_cells = true;
  e->cellstate_serial++;
  return artis_amd_populate_cellcache(e, nullptr);
}

}  // namespace

extern "C" {

int artis_amd_set_cellstate(artis_amd_engine *e, const artis_cellstate *cells, const artis_timestep *ts) {
  if (!e || !cells || !ts) {
    g_last_error = "null argument";
    return ARTIS_ERR_ARG;
  }
  const int rc = cellstate_upload(e, cells, ts, false);
  if (rc != ARTIS_OK) return rc;
  return cellstate_finish(e);
}

}  // extern "C"

extern "C" {

int artis_amd_engine_config(artis_amd_engine *e, artis_amd_config *effective) {
  if (!e || !effective) {
    g_last_error = "null argument";
    return ARTIS_ERR_ARG;
  }
  const size_t n = effective->struct_size;
  if (n > sizeof(artis_amd_config) || n < sizeof(size_t)) {
    g_last_error = "artis_amd_config.struct_size is not one this library knows: artis_amd_config_default() fills it in";
    return ARTIS_ERR_ARG;
  }
  artis_amd_config c;
  config_set_default(&c);
  c.struct_size = n;
  c.cache_budget_bytes = (int64_t)e->cache_budget;
  c.cache_headroom_bytes = (int64_t)e->cfg.cache_headroom;
  c.pop_scratch_bytes = (int64_t)e->cfg.pop_scratch;
  c.ma_hot_fraction = e->ma_hotfrac;
  c.ma_pool_fraction = e->cfg.ma_pool;
  c.tail_threshold = e->tail_max;
  c.tile_park_at = e->park_at;
  c.keep_line_dpop = e->Mh.ndpop > 0 ? 1 : 0;
  std::memcpy(effective, &c, n);
  return ARTIS_OK;
}

int artis_amd_engine_plan(const artis_model *model, int device, const artis_amd_config *cfg, int64_t free_bytes, artis_amd_plan *plan) {
  if (!model || !plan || free_bytes < 0) {
    g_last_error = !model || !plan ? "null argument" : "free_bytes is negative (0: ask the device)";
    return ARTIS_ERR_ARG;
  }
  const size_t n = plan->struct_size;
  if (n > sizeof(artis_amd_plan) || n < sizeof(size_t)) {
    g_last_error = "artis_amd_plan.struct_size is not one this library knows: set it to sizeof(artis_amd_plan)";
    return ARTIS_ERR_ARG;
  }
  artis_amd_config checked;
  if (const int rc = config_copy_checked(cfg, &checked, &g_last_error)) return rc;
  if (const int rc = validate_model(model)) return rc;
  const EngineConfig rcfg = resolve_config(checked);
  double free_b = (double)free_bytes;
  if (free_bytes == 0) {  // what a creation would find free at this moment
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
      g_last_error = "no HIP device: artis_amd_engine_plan() needs one to ask for the free memory (free_bytes = 0)";
      return ARTIS_ERR_NODEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    size_t f = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&f, &total_b));
    free_b = (double)f;
  }
  ModelOwned own;
  DevModel h;
  double hot = 1.;
  choose_record_tiers(*model, own, rcfg, free_b, &h, &hot);
  const int64_t model_bytes = model_table_bytes(h);
  CacheLayout L;
  if (const int rc = plan_cache_rows(h, rcfg, std::max(0., free_b - (double)model_bytes), &L)) return rc;
  if (L.drop_dpop) h.ndpop = 0;
  artis_amd_plan p;
  std::memset(&p, 0, sizeof(p));
  p.struct_size = n;
  p.bytes_per_cell = (int64_t)L.per_cell;
  p.cells_resident = L.tile_cells;
  p.ntiles = L.ntiles;
  p.ncold_levels = h.ncold;
  p.hot_fraction = hot;
  p.pool_slots = h.ma_pool_slots;
#define SZ(f, T, per) p.cache_bytes += (int64_t)sizeof(T) * (L.tile_cells * (int64_t)(per) + MAREC_SLACK);
  ARTIS_CACHE_ARRAYS(SZ, h)
#undef SZ
  p.pool_bytes = (int64_t)sizeof(U4) * (L.tile_cells * (int64_t)h.ma_pool_slots + MAREC_SLACK);
  p.pop_scratch_bytes = (int64_t)pop_scratch_alloc_bytes(h, pop_batch_cells(h, L.tile_cells, rcfg));
  p.model_bytes = model_bytes;
  p.free_bytes_assumed = (int64_t)free_b;
  p.line_dpop_kept = h.ndpop > 0 ? 1 : 0;
  std::memcpy(plan, &p, n);
  return ARTIS_OK;
}

int artis_amd_packets_upload(artis_amd_engine *e, const artis_packet *packets, int64_t npackets) {
  if (!e || (!packets && npackets > 0) || npackets < 0 || npackets > 2147483000LL) {
    g_last_error = "bad packet buffer";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  int rc = ensure_packet_buffers(e, npackets);
  if (rc != ARTIS_OK) return rc;
  rc = ensure_aos(e, npackets);
  if (rc != ARTIS_OK) return rc;
  if (npackets > 0) HIP_TRY(hipMemcpy(e->d_aos, packets, sizeof(artis_packet) * (size_t)npackets, hipMemcpyHostToDevice));
  return install_resident_aos(e, npackets);
}

int artis_amd_packets_download(artis_amd_engine *e, artis_packet *packets, int64_t npackets) {
  if (!e || npackets != e->npackets || (!packets && npackets > 0)) {
    g_last_error = "packet count does not match the resident population";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (npackets == 0) return ARTIS_OK;
  int rc = ensure_aos(e, npackets);
  if (rc != ARTIS_OK) return rc;
  // the fields this path never touches keep the values the caller uploaded: the structs are still on the device from
  // artis_amd_packets_upload() (no second trip over PCIe: 256 B per packet); copied again only if that buffer was replaced
  if (!e->aos_valid) HIP_TRY(hipMemcpy(e->d_aos, packets, sizeof(artis_packet) * (size_t)npackets, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_rec_to_aos, dim3(nblocks(npackets)), dim3(BLOCK), 0, nullptr, e->P, e->d_aos, e->use_perm ? e->d_perm : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(packets, e->d_aos, sizeof(artis_packet) * (size_t)npackets, hipMemcpyDeviceToHost));
  return ARTIS_OK;
}

int artis_amd_packets_snapshot(artis_amd_engine *e) {
  if (!e || !e->d_pkt) {
    g_last_error = "no resident packets";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (!e->d_pkt_snapshot) HIP_TRY(hipMalloc(&e->d_pkt_snapshot, e->pkt_bytes));
  HIP_TRY(hipMemcpy(e->d_pkt_snapshot, e->d_pkt, e->pkt_bytes, hipMemcpyDeviceToDevice));
  return ARTIS_OK;
}

int artis_amd_packets_restore(artis_amd_engine *e) {
  if (!e || !e->d_pkt || !e->d_pkt_snapshot) {
    g_last_error = "no snapshot";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(e->d_pkt, e->d_pkt_snapshot, e->pkt_bytes, hipMemcpyDeviceToDevice));
  return ARTIS_OK;
}

int artis_amd_estimators_zero(artis_amd_engine *e, void *hip_stream) {
  if (!e) return ARTIS_ERR_ARG;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemsetAsync(e->d_est, 0, sizeof(double) * (size_t)e->est_ndoubles, (hipStream_t)hip_stream));
  HIP_TRY(hipMemsetAsync(e->d_stats, 0, sizeof(unsigned long long) * ARTIS_NSTATS, (hipStream_t)hip_stream));
  // (d_bfrate_kept is zero between calls: k_bfrate_expand leaves it so)
  return ARTIS_OK;
}

int artis_amd_estimators_download(artis_amd_engine *e, artis_estimators *est) {
  if (!e || !est) return ARTIS_ERR_ARG;
  HIP_TRY(hipSetDevice(e->device));
  std::vector<double> h((size_t)e->est_ndoubles);
  HIP_TRY(hipMemcpy(h.data(), e->d_est, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  const int64_t ncell = e->Mh.npts_nonempty;
  const int64_t g = e->Mh.nbfcontinua_ground > 0 ? e->Mh.nbfcontinua_ground : 1;
  const double *src = h.data();
  auto add = [](double *dst, const double *s, int64_t cnt) {
    if (!dst) return;
    for (int64_t i = 0; i < cnt; i++) dst[i] += s[i];
  };
  auto add_strided = [](double *dst, const double *s, int64_t cnt, int64_t stride) {
    if (!dst) return;
    for (int64_t i = 0; i < cnt; i++) dst[i] += s[i * stride];
  };
  add_strided(est->J, src, ncell, 8);
  add_strided(est->nuJ, src + 1, ncell, 8);
  add_strided(est->ffheatingestimator, src + 2, ncell, 8);
  add_strided(est->colheatingestimator, src + 3, ncell, 8);
  add_strided(est->dep_estimator_gamma, src + 4, ncell, 8);
  add_strided(est->dep_estimator_electron, src + 5, ncell, 8);
  add_strided(est->dep_estimator_positron, src + 6, ncell, 8);
  add_strided(est->dep_estimator_alpha, src + 7, ncell, 8);
  add_strided(est->gammaestimator, src + 8 * ncell, ncell * g, 2);
  add_strided(est->bfheatingestimator, src + 8 * ncell + 1, ncell * g, 2);
  add(est->scalars, src + 8 * ncell + 2 * ncell * g, ARTIS_NSCALARS);
  {
    const int64_t nbinest = ARTIS_OPT_MULTIBIN_RADFIELD_MODEL_ON ? ncell * ARTIS_OPT_RADFIELDBINCOUNT : 0;
    const int64_t nbfest = ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON ? ncell * (int64_t)e->Mh.nbfestim : 0;
    const double *ext = src + 8 * ncell + 2 * ncell * g + ARTIS_NSCALARS;
    if (nbinest) {
      add_strided(est->radfieldbin_J, ext, nbinest, 2);
      add_strided(est->radfieldbin_nuJ, ext + 1, nbinest, 2);
    }
    if (nbfest) add(est->bfrate_raw, ext + 2 * nbinest, nbfest);
    const int64_t nlineest = ARTIS_OPT_DETAILED_LINE_ESTIMATORS_ON ? ncell * (int64_t)e->Mh.detailed_linecount : 0;
    if (nlineest) {
      add(est->Jb_lu_raw, ext + 2 * nbinest + nbfest, nlineest);
      if (est->Jb_lu_contribcount)
        for (int64_t i = 0; i < nlineest; i++) est->Jb_lu_contribcount[i] += (int64_t)ext[2 * nbinest + nbfest + nlineest + i];
    }
    if (e->nvspec) add(est->vspecpol, ext + 2 * nbinest + nbfest + 2 * nlineest, e->nvspec);
    if (e->nvgrid) add(est->vgrid_flux, ext + 2 * nbinest + nbfest + 2 * nlineest + e->nvspec, e->nvgrid);
  }
  if (est->stats) {
    unsigned long long st[ARTIS_NSTATS];
    HIP_TRY(hipMemcpy(st, e->d_stats, sizeof(st), hipMemcpyDeviceToHost));
    for (int i = 0; i < ARTIS_NSTATS; i++) est->stats[i] += (int64_t)st[i];
  }
  return ARTIS_OK;
}

int artis_amd_estimators_devptr(artis_amd_engine *e, void **dptr, int64_t *ndoubles) {
  if (!e || !dptr || !ndoubles) return ARTIS_ERR_ARG;
  *dptr = e->d_est;
  *ndoubles = e->est_ndoubles;
  return ARTIS_OK;
}

int artis_amd_comm_unique_id(void *id_out) {
  if (!id_out) return ARTIS_ERR_ARG;
  if (!rccl_api().ok) {
    g_last_error = "librccl could not be loaded";
    return ARTIS_ERR_RCCL;
  }
  ncclUniqueId id;
  RCCL_TRY(rccl_api().GetUniqueId(&id));
  std::memcpy(id_out, id.internal, ARTIS_AMD_COMM_ID_BYTES);
  return ARTIS_OK;
}

int artis_amd_comm_init(artis_amd_engine *e, int nranks, int rank, const void *id_bytes) {
  if (!e || !id_bytes || nranks < 1 || rank < 0 || rank >= nranks) {
    g_last_error = "bad communicator arguments";
    return ARTIS_ERR_ARG;
  }
  if (!rccl_api().ok) {
    g_last_error = "librccl could not be loaded";
    return ARTIS_ERR_RCCL;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (e->comm) {
    (void)rccl_api().CommDestroy(e->comm);
    e->comm = nullptr;
  }
  ncclUniqueId id;
  std::memcpy(id.internal, id_bytes, ARTIS_AMD_COMM_ID_BYTES);
  RCCL_TRY(rccl_api().CommInitRank(&e->comm, nranks, id, rank));
  return ARTIS_OK;
}

int artis_amd_comm_count(artis_amd_engine *e, void *nccl_comm, int *nranks) {
  if (!e || !nranks) return ARTIS_ERR_ARG;
  ncclComm_t comm = nccl_comm ? (ncclComm_t)nccl_comm : e->comm;
  if (!comm || !rccl_api().ok || !rccl_api().CommCount) {
    g_last_error = "no communicator (artis_amd_comm_init), or librccl without ncclCommCount";
    return ARTIS_ERR_RCCL;
  }
  RCCL_TRY(rccl_api().CommCount(comm, nranks));
  return ARTIS_OK;
}

int artis_amd_allreduce_estimators(artis_amd_engine *e, void *nccl_comm, void *hip_stream) {
  if (!e) return ARTIS_ERR_ARG;
  ncclComm_t comm = nccl_comm ? (ncclComm_t)nccl_comm : e->comm;
  if (!comm) {
    g_last_error = "no communicator: pass an ncclComm_t or call artis_amd_comm_init() first";
    return ARTIS_ERR_ARG;
  }
  if (!rccl_api().ok) {
    g_last_error = "librccl could not be loaded";
    return ARTIS_ERR_RCCL;
  }
  HIP_TRY(hipSetDevice(e->device));
  // one in-place sum over the whole block [J | nuJ | ffheat | colheat | gamma | bfheat | dep_* | scalars]
  RCCL_TRY(rccl_api().AllReduce(e->d_est, e->d_est, (size_t)e->est_ndoubles, ncclDouble, ncclSum, comm, (hipStream_t)hip_stream));
  return ARTIS_OK;
}

int artis_amd_update_packets(artis_amd_engine *e, artis_packet *packets, int64_t npackets, artis_estimators *est) {
  int rc = artis_amd_packets_upload(e, packets, npackets);
  if (rc != ARTIS_OK) return rc;
  rc = artis_amd_estimators_zero(e, nullptr);
  if (rc != ARTIS_OK) return rc;
  {
    // keep UPDATECELL of the populate that belongs to this timestep (with several cache tiles the populates happen
    // inside the update and count themselves)
    unsigned long long ncell = (e->cc.ntiles == 1) ? (unsigned long long)e->Mh.npts_nonempty : 0ull;
    HIP_TRY(hipMemcpy(e->d_stats + ARTIS_STAT_UPDATECELL, &ncell, sizeof(ncell), hipMemcpyHostToDevice));
  }
  rc = artis_amd_update_packets_device(e, nullptr);
  if (rc != ARTIS_OK) return rc;
  rc = artis_amd_packets_download(e, packets, npackets);
  if (rc != ARTIS_OK) return rc;
  if (est) rc = artis_amd_estimators_download(e, est);
  return rc;
}

int artis_amd_last_kernel_ms(artis_amd_engine *e, double *propagate_ms, int64_t *nlaunches) {
  if (!e) return ARTIS_ERR_ARG;
  if (propagate_ms) *propagate_ms = e->last.propagate_ms;
  if (nlaunches) *nlaunches = e->last.nlaunches;
  return ARTIS_OK;
}

int artis_amd_last_kernel_launches(artis_amd_engine *e, int64_t *rpkt_launches, int64_t *thermal_launches) {
  if (!e) return ARTIS_ERR_ARG;
  if (rpkt_launches) *rpkt_launches = e->last.klaunches[NEXT_RPKT];
  if (thermal_launches) *thermal_launches = e->last.klaunches[NEXT_MA] + e->last.klaunches[NEXT_KPKT];
  return ARTIS_OK;
}

int artis_amd_last_kernel_breakdown(artis_amd_engine *e, double *rpkt_ms, int64_t *rpkt_threads, double *thermal_ms,
                                    int64_t *thermal_threads) {
  if (!e) return ARTIS_ERR_ARG;
  if (rpkt_ms) *rpkt_ms = e->last.kms[NEXT_RPKT];
  if (rpkt_threads) *rpkt_threads = e->last.kthreads[NEXT_RPKT];
  if (thermal_ms) *thermal_ms = e->last.kms[NEXT_MA] + e->last.kms[NEXT_KPKT];
  if (thermal_threads) *thermal_threads = e->last.kthreads[NEXT_MA] + e->last.kthreads[NEXT_KPKT];
  return ARTIS_OK;
}

int artis_amd_last_tiling_fills(artis_amd_engine *e, int64_t *sparse_fills, int64_t *cells_filled) {
  if (!e) return ARTIS_ERR_ARG;
  if (sparse_fills) *sparse_fills = e->last.sparse_fills;
  if (cells_filled) *cells_filled = e->last.cells_filled;
  return ARTIS_OK;
}

int artis_amd_last_pool_resets(artis_amd_engine *e, int64_t *resets) {
  if (!e) return ARTIS_ERR_ARG;
  if (resets) *resets = e->last.pool_resets;
  return ARTIS_OK;
}

int artis_amd_record_tiers(artis_amd_engine *e, double *hot_fraction, int32_t *ncold_levels, int64_t *pool_slots) {
  if (!e) return ARTIS_ERR_ARG;
  if (hot_fraction) *hot_fraction = e->ma_hotfrac;
  if (ncold_levels) *ncold_levels = e->Mh.ncold;
  if (pool_slots) *pool_slots = e->Mh.ma_pool_slots;
  return ARTIS_OK;
}
int artis_amd_last_pool_usage(artis_amd_engine *e, int64_t *units_used, int64_t *units_cap) {
  if (!e) return ARTIS_ERR_ARG;
  if (units_used) *units_used = e->last_pool_used;
  if (units_cap) *units_cap = e->last_pool_cap;
  return ARTIS_OK;
}
int artis_amd_last_absent_records(artis_amd_engine *e, int64_t *skipped, int64_t *filled) {
  if (!e) return ARTIS_ERR_ARG;
  if (skipped) *skipped = e->last_absent_skipped;
  if (filled) *filled = e->last_absent_filled;
  return ARTIS_OK;
}
int artis_amd_last_thermal_variants(artis_amd_engine *e, int32_t *mask) {
  if (!e || !mask) return ARTIS_ERR_ARG;
  *mask = e->last.thermal_variants;
  return ARTIS_OK;
}
int artis_amd_last_estimator_forms(artis_amd_engine *e, int32_t *mask) {
  if (!e || !mask) return ARTIS_ERR_ARG;
  *mask = e->last.est_forms;
  return ARTIS_OK;
}
int artis_amd_last_tiling_parked(artis_amd_engine *e, int64_t *parked) {
  if (!e) return ARTIS_ERR_ARG;
  if (parked) *parked = e->last.parked;
  return ARTIS_OK;
}

int artis_amd_last_tiling(artis_amd_engine *e, int64_t *sweeps, int64_t *tile_fills, double *fill_ms, int64_t *listed) {
  if (!e) return ARTIS_ERR_ARG;
  if (sweeps) *sweeps = e->last.sweeps;
  if (tile_fills) *tile_fills = e->last.tile_fills;
  if (fill_ms) *fill_ms = e->last.fill_ms;
  if (listed) *listed = e->last.listed;
  return ARTIS_OK;
}

int artis_amd_last_kernel_table(artis_amd_engine *e, double ms[4], int64_t launches[4], int64_t packets[4]) {
  if (!e) return ARTIS_ERR_ARG;
  const int kinds[4] = {NEXT_RPKT, NEXT_MA, NEXT_KPKT, NEXT_SLOW};
  for (int i = 0; i < 4; i++) {
    if (ms) ms[i] = e->last.kms[kinds[i]];
    if (launches) launches[i] = e->last.klaunches[kinds[i]];
    if (packets) packets[i] = e->last.kthreads[kinds[i]];
  }
  return ARTIS_OK;
}

int artis_amd_last_kernel_ms_by_kind(artis_amd_engine *e, double ms[8], int64_t launches[8]) {
  if (!e || !ms) return ARTIS_ERR_ARG;
  const int kinds[5] = {NEXT_RPKT, NEXT_MA, NEXT_SLOW, NEXT_GAMMA, NEXT_BB};
  for (int i = 0; i < 8; i++) {
    ms[i] = 0.;
    if (launches) launches[i] = 0;
  }
  for (int i = 0; i < 5; i++) {
    ms[i] = e->last.kms[kinds[i]];
    if (launches) launches[i] = e->last.klaunches[kinds[i]];
  }
  ms[5] = e->last.kms_tail;
  ms[6] = e->last.fill_ms;
  ms[7] = e->last.kms_late;
  if (launches) {
    launches[5] = e->last.tail_launches;
    launches[7] = e->last.late_launches;
  }
  return ARTIS_OK;
}

int artis_amd_debug_visit_counts(artis_amd_engine *e, uint32_t *counts, int64_t n) {
  if (!e || !counts || n != (int64_t)e->Mh.npts_nonempty * e->Mh.nlevels) {
    g_last_error = "visit counts: [npts_nonempty][nlevels] uint32 expected";
    return ARTIS_ERR_ARG;
  }
  if (e->d_visit_counts == nullptr) {
    g_last_error = "this library was not built with -DARTIS_VISIT_COUNTS (or no propagation call has run yet)";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpy(counts, e->d_visit_counts, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return ARTIS_OK;
}

int artis_amd_debug_sort_list(artis_amd_engine *e, const int32_t *keys, const int32_t *list, int32_t n, int64_t nkeys, int32_t *out) {
  if (!e || n < 0 || (n > 0 && (!keys || !list || !out))) {
    g_last_error = "null argument or negative length";
    return ARTIS_ERR_ARG;
  }
  if (nkeys <= SORT_LDS_KEYS) {
    g_last_error = "debug_sort_list runs the many-keys sort: nkeys has to be above " + std::to_string(SORT_LDS_KEYS);
    return ARTIS_ERR_ARG;
  }
  if (nkeys > SORT_MAX_KEYS) {
    g_last_error = sort_too_many_keys_text(nkeys);
    return ARTIS_ERR_UNSUPPORTED;
  }
  for (int32_t i = 0; i < n; i++)
    if (keys[i] < 0 || keys[i] >= nkeys) {
      g_last_error = "a key is outside [0, nkeys)";
      return ARTIS_ERR_ARG;
    }
  if (n < 2 * BLOCK) {  // sort_by_key() leaves so short a list as it is
    if (n > 0) std::memcpy(out, list, sizeof(int32_t) * (size_t)n);
    return ARTIS_OK;
  }
  HIP_TRY(hipSetDevice(e->device));
  // the engine's own sort scratch (grown if this list is longer than its packet lists: it holds nothing between two sorts), buffers of the
  // call's own for keys, list and output: the engine's lists are not touched
  SortScratch &S = e->sort_scratch;
  int32_t *d_io = nullptr;  // keys, list, out
  int rc = (S.capacity >= n) ? ARTIS_OK : sort_scratch_alloc(S, n);
  if (rc == ARTIS_OK && hipMalloc((void **)&d_io, sizeof(int32_t) * 3 * (size_t)n) != hipSuccess) {
    g_last_error = "debug_sort_list: out of device memory";
    rc = ARTIS_ERR_HIP;
  }
  auto copy = [&](void *dst, const void *src, hipMemcpyKind kind) {
    if (rc == ARTIS_OK && hipMemcpy(dst, src, sizeof(int32_t) * (size_t)n, kind) != hipSuccess) {
      g_last_error = "debug_sort_list: copy failed";
      rc = ARTIS_ERR_HIP;
    }
  };
  copy(d_io, keys, hipMemcpyHostToDevice);
  copy(d_io + n, list, hipMemcpyHostToDevice);
  if (rc == ARTIS_OK) rc = sort_many_keys(e, S, nullptr, d_io + n, d_io, n, nkeys, d_io + 2 * (size_t)n);
  if (rc == ARTIS_OK && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) {
    g_last_error = "debug_sort_list: a sort kernel failed";
    rc = ARTIS_ERR_HIP;
  }
  copy(out, d_io + 2 * (size_t)n, hipMemcpyDeviceToHost);
  if (d_io) (void)hipFree(d_io);
  return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ the cell cache's host side; the propagation driver; the timestep-end stages: spectra, radiation-field fit, ion balance, decay update, deposition rates; the pellet initialisation; thermal balance and its bound-free heating coefficients
#include "stage_cellcache.h"
#include "stage_propagate.h"
#include "stage_common.h"
#include "stage_spectra.h"
#include "stage_radfield.h"
#include "stage_ionbal.h"
#include "stage_decay.h"
#include "stage_deposition.h"
#include "stage_packet_init.h"
#include "stage_thermal.h"
#include "stage_bfheat.h"
#include "stage_ratecoeff.h"
#include "stage_photoion.h"
