// list_kernels.h -- the kernels between the caller's packets and the engine's records (k_aos_to_rec, k_rec_to_aos, k_aos_cellkeys), the work lists
// (Lists, append_by_kind) and the kernels that fill and count them (k_classify, k_count_waiting). Included by artis_engine.hip inside its anonymous namespace,
// after cellcache_kernels.h.
#pragma once
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
