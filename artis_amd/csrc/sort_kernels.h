// sort_kernels.h -- the counting sorts of a work list by (cell, frequency bin): the tile histogram / plan / segment passes for many keys, the scan
// kernels, and the one-pass LDS form for few keys. Included by artis_engine.hip inside its anonymous namespace; the host side is sort_list() in artis_engine.hip.
#pragma once
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
