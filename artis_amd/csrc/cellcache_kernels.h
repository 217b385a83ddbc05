// cellcache_kernels.h -- the kernels that populate the cell cache (tables.h DevCache) and their device helpers; ma_fill_record_wave / ma_fill_wave
// are also what k_slow and k_tail fill a cold level's record with. Included by artis_engine.hip inside its anonymous namespace, before the packet
// and propagation kernels; the host side that launches them is stage_cellcache.h.
#pragma once
// ------------------------------------------------------------------ populate kernels
// The cells a fill works on: every cell (the whole cache at once, or a batch of it), or -- a tiled cache (Env::fill_cells) -- the listed ones: the cells
// make_resident() gave rows to.
__device__ inline int64_t fill_count(const Env &env) { return env.fill_cells ? env.nfill : (env.tile_hi - env.tile_lo); }
__device__ inline int fill_cell(const Env &env, int64_t k) { return env.fill_cells ? env.fill_cells[k] : env.tile_lo + (int)k; }
#ifndef ARTIS_MA_WAVE_FILL
#define ARTIS_MA_WAVE_FILL 1  // a cold level's record filled by the wave (ma_fill_record_wave); 0: by the lane (physics.h ma_fill_record)
#endif
#ifndef ARTIS_COLD_COOLING_ONLY
#define ARTIS_COLD_COOLING_ONLY 1  // the population evaluates of a cold level's transitions only the cooling terms (physics.h matrans_terms<true>)
#endif
__global__ void __launch_bounds__(BLOCK) k_levelpops(Env env) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t total = fill_count(env) * env.M.nlevels;
  if (i >= total) return;
  populate_levelpop(env, fill_cell(env, i / env.M.nlevels), (int)(i % env.M.nlevels));
}
// ABSENT IONS (tables.h): which ions the population of the macro-atom records leaves out in each cell of the fill. After k_levelpops, from the
// populations the kernels below read (whoever formed them). One WAVE per cell, a LANE per ion: the lane adds its ion's populations up (the wave's
// lanes read one row: its lines are fetched once) and leaves the sum in the row's own scratch (Env::ion_popsum), then -- the wave's lanes together
// again, their stores done -- compares it with its element's sum. `<=` with the product: an element without abundance is wholly absent, eps = 0 means "exactly zero",
// eps = 1 every ion. counts[0] += the static records left out (an ion's static records are those of its lowest levels: model_build.h).
__global__ void __launch_bounds__(BLOCK) k_ion_absent(Env env) {
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= fill_count(env)) return;
  const DevModel &M = env.M;
  const int c = fill_cell(env, wave);
  const double *pops = env.K.levelpops + (krow(env, c) * M.nlevels);
  double *ionsum = env.ion_popsum + (krow(env, c) * M.nions);
  uint8_t *absent = env.ion_absent + (krow(env, c) * M.nions);
  for (int ui = lane; ui < M.nions; ui += 64) {
    const int start = M.ion_uniquelevelindexstart[ui], n = M.ion_nlevels[ui];
    double s = 0.;
    for (int l = 0; l < n; l++) s += pops[start + l];
    ionsum[ui] = s;
  }
  // the lanes read each other's sums below: every lane of the wave has left the loop above (the barrier) and its stores are visible (the fence)
  __builtin_amdgcn_wave_barrier();
  __threadfence();
  __builtin_amdgcn_wave_barrier();
  unsigned int nskip = 0;
  for (int ui = lane; ui < M.nions; ui += 64) {
    const int element = M.ion_element[ui];
    const int i0 = M.elem_uniqueionindexstart[element], ni = M.elem_nions[element];
    double total = 0.;
    for (int i = 0; i < ni; i++) total += ionsum[i0 + i];
    const bool a = ionsum[ui] <= env.ma_absent_eps * total;
    absent[ui] = a ? 1 : 0;
    if (a) {  // the ion's levels with a static record: the first lo of them (bisection for the first cold level)
      const int start = M.ion_uniquelevelindexstart[ui];
      int lo = 0, hi = M.ion_nlevels[ui];
      while (lo < hi) {
        const int mid = lo + ((hi - lo) / 2);
        if (M.level_pack[start + mid].rec_off >= 0) lo = mid + 1; else hi = mid;
      }
      nskip += (unsigned int)lo;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nskip += __shfl_xor(nskip, o);
  if (lane == 0 && nskip != 0) atomicAdd(env.ma_absent_counts, (unsigned long long)nskip);
}
__global__ void __launch_bounds__(BLOCK) k_line_dpop(Env env) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t total = fill_count(env) * env.M.nlines;
  if (i >= total) return;
  populate_line_dpop(env, fill_cell(env, i / env.M.nlines), (int)(i % env.M.nlines));
}
#if ARTIS_EXPOPAC_TABLES
// calculate_expansion_opacities() for the cells of the resident tile, when the host did not hand the tables over
__global__ void __launch_bounds__(BLOCK) k_expopac(Env env) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t total = fill_count(env) * ARTIS_EXPOPAC_NBINS;
  if (i >= total) return;
  const int c = fill_cell(env, i / ARTIS_EXPOPAC_NBINS);
  if (env.C.thick[c] == ARTIS_CELL_THICK) return;  // update_grid.cc:657
  populate_expopac_bin(env, c, (int)(i % ARTIS_EXPOPAC_NBINS));
}
__global__ void __launch_bounds__(BLOCK) k_expopac_planck(Env env) {
  const int64_t kf = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (kf >= fill_count(env)) return;
  const int c = fill_cell(env, kf);
  if (env.C.thick[c] == ARTIS_CELL_THICK) return;
  populate_expopac_planck(env, c);
}
#endif
#if ARTIS_OPT_NT_ON
// every cell of the model (not a tile): the non-thermal ionisation rate coefficients and energy-rate sums
__global__ void __launch_bounds__(BLOCK) k_nt_cells(Env env, int ncell) {
  const int c = blockIdx.x * BLOCK + threadIdx.x;
  if (c >= ncell) return;
  if (!populate_nt_cell(env, c)) fail(env, 90);
}
#endif
__global__ void __launch_bounds__(BLOCK) k_cell_scalars(Env env) {
  const int64_t kf = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (kf >= fill_count(env)) return;
  const int c = fill_cell(env, kf);
  populate_chi_ff(env, c);
}
// one wave = one 64-bit word of a cell's keep bitmap: the ballot IS the word (globals.h:296-305)
__global__ void __launch_bounds__(BLOCK) k_allcont(Env env) {
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = fill_count(env) * env.M.nkeepwords;
  if (wave >= nwaves) return;
  const int c = fill_cell(env, wave / env.M.nkeepwords);
  const int word = (int)(wave % env.M.nkeepwords);
  const int i = word * 64 + lane;
  bool keep = false;
  if (i < env.M.nbfcontinua) keep = populate_allcont(env, c, i);
  const unsigned long long bits = __ballot(keep);
  if (lane == 0) env.K.allcont_keepbits[(krow(env, c) * env.M.nkeepwords) + word] = bits;
}
// one wave = one cell: the kept continua as a list, the count of kept continua below each bitmap word and the pairs in list
// order (physics.h populate_keptlist; after k_allcont)
__global__ void __launch_bounds__(BLOCK) k_keptlist(Env env) {
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= fill_count(env)) return;
  const int c = fill_cell(env, wave);
  const int nw = env.M.nkeepwords;
  const uint64_t *keep = env.K.allcont_keepbits + (krow(env, c) * nw);
  int32_t *list = env.K.allcont_keptlist + (krow(env, c) * env.M.nbfcontinua);
  int32_t *prefix = env.K.allcont_keepprefix + (krow(env, c) * nw);
  const D2 *pair = env.K.allcont_pair + (krow(env, c) * env.M.nbfcontinua);
  D2 *keptpair = env.K.allcont_keptpair + (krow(env, c) * env.M.nbfcontinua);
  int base = 0;
  for (int w0 = 0; w0 < nw; w0 += 64) {
    const int j = w0 + lane;
    unsigned long long word = (j < nw) ? keep[j] : 0ull;
    const int pc = __popcll(word);
    int incl = pc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    int at = base + incl - pc;
    if (j < nw) prefix[j] = at;
    while (word != 0ull) {
      const int i = (j * 64) + __builtin_ctzll(word);
      list[at] = i;
      keptpair[at] = pair[i];
      at++;
      word &= word - 1ull;
    }
    base += __shfl(incl, 63);
  }
}
__global__ void __launch_bounds__(BLOCK) k_corrphotoion(Env env, const int32_t *target_level) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t total = fill_count(env) * env.M.nphixstargets_total;
  if (i >= total) return;
  const int c = fill_cell(env, i / env.M.nphixstargets_total);
  const int k = (int)(i % env.M.nphixstargets_total);
  const int ul = target_level[k];
  populate_corrphotoion(env, c, ul, k - env.M.level_phixstargetstart[ul]);
}
// Bound-bound part of a cell's macro-atom records: one WAVE per (cell, block of alltrans entries), three passes over the
// block's entries in LDS (round 4; rounds 2-3: a wave scan in registers whose serial steps -- one per position in the longest
// segment of a 64-entry chunk, 18 instructions each for all 64 lanes -- were 11 % of the population with ~9 transitions per
// direction and 26 % with ~25):
//   1. every lane evaluates the rate coefficients of its transitions (every lane busy, whatever the levels' transition counts)
//      and leaves the three terms each adds to its level's running sums (macroatom.cc:64-140) in LDS;
//   2. ONE LANE PER SEGMENT (a level's downward or upward transitions) adds its segment's terms up in the reference's order --
//      the additions of the sequential form (physics.h populate_level_bb / populate_dirfilter_seq), so the same bits -- 10-30
//      segments side by side, and writes the level's rates;
//   3. every lane turns its transitions' sums into filter entries (tables.h "FILTERS": fractions of the segment's last sum); a
//      line is usable when every one of its entries is a finite fraction (a flag per line in LDS).
// A segment longer than a block (DevModel::malongsegs) is a block of its own: its rates are summed here 64 terms at a time, its
// filters written by k_mafilter_long.
// the value of the lane below (lane 0: 0), as two DPP wave-shift moves
__device__ inline double wave_shr1(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// the lanes of the wave that hold the entries of this lane's filter line (7 transitions of one direction: consecutive lanes)
__device__ inline unsigned long long line_lanes(int lane, int ti, int seglen) {
  const int first = lane - (ti % MAREC_PER);
  const int left = seglen - (ti - (ti % MAREC_PER));
  const int cnt = left < MAREC_PER ? left : MAREC_PER;
  return ((1ull << cnt) - 1ull) << first;
}
// where entry e of a block (alltrans index a0 + e) sits in its segment
struct MaEntryPos {
  LevelPack lpk;
  int ti, seglen, e_seg0;  // index within the direction, the direction's transitions, the block entry of the direction's first
  bool isdown;
};
__device__ inline MaEntryPos ma_entry_pos(const DevModel &M, int a0, int e) {
  MaEntryPos r;
  r.lpk = M.level_pack[M.alltrans_owner[a0 + e]];
  const int i = (a0 + e) - r.lpk.alltrans_startdown;
  r.isdown = i < r.lpk.ndown;
  r.ti = r.isdown ? i : i - r.lpk.ndown;
  r.seglen = r.isdown ? r.lpk.ndown : r.lpk.nup;
  r.e_seg0 = e - r.ti;
  return r;
}
__global__ void __launch_bounds__(BLOCK, 4) k_matrans(Env env) {
  __shared__ double lds_v[BLOCK / 64][3][MATRANS_BLOCK];          // the terms, then the running sums
  __shared__ uint16_t lds_q[BLOCK / 64][2][MATRANS_BLOCK];        // filter entries: internal, radiative
  __shared__ uint8_t lds_qf[BLOCK / 64][MATRANS_BLOCK];           // ... the internal entries' fine bytes (tables.h "FINE BYTES")
  __shared__ uint8_t lds_ok[BLOCK / 64][2][MATRANS_BLOCK];        // per filter line (at its first entry): every entry a finite fraction
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const DevModel &M = env.M;
  const int nblk = M.nscanblk;
  if (wave >= fill_count(env) * nblk) return;
  const int64_t kf = wave / nblk;
  const int c = fill_cell(env, kf);
  const int blk = (int)(wave % nblk);
  const int seg0 = M.scanblk_seg0[blk], seg1 = M.scanblk_seg0[blk + 1];
  const MaLongSeg sfirst = M.scansegs[seg0], slast = M.scansegs[seg1 - 1];
  const int a0 = sfirst.ats0, nent = (slast.ats0 + slast.n) - a0;
  U4 *row = env.K.macache + (krow(env, c) * M.nmacache);
  double *upterms = env.collexc_terms + (kf * M.nupcum);
  double(*v)[MATRANS_BLOCK] = lds_v[w];
  // ABSENT IONS (tables.h): a block that lies inside one ion (levels are in the order of their ions) which is absent in this cell leaves as a wave
  // with the collisional-excitation cooling terms of its upward entries alone -- the cooling list needs them, bit for bit; nothing of the records is
  // written (k_macroatom leaves the marker in them). A block that straddles ions skips its absent levels' writes below.
  const int ion_first = M.level_ion[sfirst.ul], ion_last = M.level_ion[slast.ul];
  if (ion_first == ion_last && ma_ion_absent(env, c, ion_first)) {
    for (int k = lane; k < nent; k += 64) {
      const int e = (nent > MATRANS_BLOCK) ? k : M.scanperm[a0 + k];
      const MaTransTerms t = matrans_terms<true>(env, c, a0 + e);
      if (!t.isdown) upterms[M.level_upcum_start[t.ul] + t.i] = t.kterm;
    }
    return;
  }
  if (nent > MATRANS_BLOCK) {
    // one long segment: its rates, 64 terms at a time (lane k adds its term to the finished sum of lane k - 1; lane 0 takes the carry)
    const LevelPack lpk = M.level_pack[sfirst.ul];
    double c0 = 0., c1 = 0., c2 = 0.;
    for (int base = 0; base < nent; base += 64) {
      const bool valid = base + lane < nent;
      MaTransTerms t;
      t.v0 = t.v1 = t.v2 = t.kterm = 0.;
      if (valid) {
        t = matrans_terms<ARTIS_COLD_COOLING_ONLY != 0>(env, c, a0 + base + lane);
        if (!t.isdown) upterms[M.level_upcum_start[t.ul] + t.i] = t.kterm;
      }
      double s0 = (lane == 0 ? c0 : 0.) + t.v0, s1 = (lane == 0 ? c1 : 0.) + t.v1, s2 = (lane == 0 ? c2 : 0.) + t.v2;
      for (int k = 1; k < 64; k++) {
        const double p0 = wave_shr1(s0), p1 = wave_shr1(s1), p2 = wave_shr1(s2);
        if (lane == k) {
          s0 = p0 + t.v0;
          s1 = p1 + t.v1;
          s2 = p2 + t.v2;
        }
      }
      const int last = (nent - base < 64 ? nent - base : 64) - 1;
      c0 = __shfl(s0, last);
      c1 = __shfl(s1, last);
      c2 = __shfl(s2, last);
    }
    if (lane == 0 && lpk.rec_off >= 0) {  // (a cold level has no static record: only its cooling terms above are kept)
      double *rates = ma_rates_of(row + lpk.rec_off, lpk.ndown, lpk.nup);
      if (sfirst.dir == 0) {
        rates[ARTIS_MA_ACTION_RADDEEXC] = c0;
        rates[ARTIS_MA_ACTION_COLDEEXC] = c1;
        rates[ARTIS_MA_ACTION_INTERNALDOWNSAME] = c2;
      } else {
        rates[ARTIS_MA_ACTION_INTERNALUPSAME] = c0;
      }
    }
    return;
  }
  // 1. the terms (the block's entries in the order of DevModel::scanperm: a wave's 64 entries are of one kind wherever the block has 64 of it)
  for (int k = lane; k < nent; k += 64) {
    const int e = M.scanperm[a0 + k];
    const MaTransTerms t = matrans_terms<ARTIS_COLD_COOLING_ONLY != 0>(env, c, a0 + e);
    v[0][e] = t.v0;
    v[1][e] = t.v1;
    v[2][e] = t.v2;
    lds_ok[w][0][e] = 1;
    lds_ok[w][1][e] = 1;
    if (!t.isdown) upterms[M.level_upcum_start[t.ul] + t.i] = t.kterm;
  }
  __threadfence_block();  // (the passes exchange data between the lanes of this wave through LDS: in order, but the compiler must not move them)
  // 2. the running sums, a lane per segment
  for (int si = seg0 + lane; si < seg1; si += 64) {
    const MaLongSeg sg = M.scansegs[si];
    const int o = sg.ats0 - a0;
    double s0 = 0., s1 = 0., s2 = 0.;
    for (int i = 0; i < sg.n; i++) {
      s0 += v[0][o + i];
      s1 += v[1][o + i];
      s2 += v[2][o + i];
      v[0][o + i] = s0;
      v[2][o + i] = s2;
    }
    const LevelPack lpk = M.level_pack[sg.ul];
    if (lpk.rec_off < 0 || ma_ion_absent(env, c, M.level_ion[sg.ul])) continue;
    double *rates = ma_rates_of(row + lpk.rec_off, lpk.ndown, lpk.nup);
    if (sg.dir == 0) {
      rates[ARTIS_MA_ACTION_RADDEEXC] = s0;
      rates[ARTIS_MA_ACTION_COLDEEXC] = s1;
      rates[ARTIS_MA_ACTION_INTERNALDOWNSAME] = s2;
    } else {
      rates[ARTIS_MA_ACTION_INTERNALUPSAME] = s0;
    }
  }
  __threadfence_block();
  // 3a. the filter entries of every transition: its running sums as fractions of the direction's last ones
  for (int e = lane; e < nent; e += 64) {
    const MaEntryPos ps = ma_entry_pos(M, a0, e);
    const int e_last = ps.e_seg0 + ps.seglen - 1;
    const double whole_int = v[ps.isdown ? 2 : 0][e_last], whole_rad = v[0][e_last];
    bool ok_int = (whole_int > 0.) && (whole_int <= DBLMAX), ok_rad = (whole_rad > 0.) && (whole_rad <= DBLMAX);
    uint32_t q_int = MAFILT_NONE23, q_rad = MAFILT_NONE;
    if (ps.ti < ps.seglen - 1) {
      if (ok_int) q_int = mafilt_quant23(v[ps.isdown ? 2 : 0][e], whole_int, &ok_int);
      if (ok_rad && ps.isdown) q_rad = mafilt_quant(v[0][e], whole_rad, &ok_rad);
    }
    lds_q[w][0][e] = (uint16_t)(q_int >> 8);
    lds_qf[w][e] = (uint8_t)(q_int & 0xFFu);
    lds_q[w][1][e] = (uint16_t)q_rad;
    const int e_line = e - (ps.ti % MAREC_PER);
    if (!ok_int) lds_ok[w][0][e_line] = 0;
    if (ps.isdown && !ok_rad) lds_ok[w][1][e_line] = 0;
  }
  __threadfence_block();
  // 3b. ... into the records: the entries of a line that is not usable are 0, its mark too
  for (int e = lane; e < nent; e += 64) {
    const MaEntryPos ps = ma_entry_pos(M, a0, e);
    if (ps.lpk.rec_off < 0 || ma_ion_absent(env, c, M.level_ion[M.alltrans_owner[a0 + e]])) continue;
    const int e_line = e - (ps.ti % MAREC_PER);
    U4 *rec = row + ps.lpk.rec_off;
    const bool lok_int = lds_ok[w][0][e_line] != 0;
    U4 *line = rec + marec_slot(ps.isdown ? MADIR_DOWN : MADIR_UP, ps.ti / MAREC_PER, ps.lpk.ndown, ps.lpk.nup);
    mafilt_put(line, ps.ti % MAREC_PER, lok_int ? lds_q[w][0][e] : 0u);
    ((uint8_t *)rec)[marec_fine_byte0(ps.isdown ? MADIR_DOWN : MADIR_UP, ps.ti / MAREC_PER, ps.lpk.ndown, ps.lpk.nup) + (ps.ti % MAREC_PER)] =
        lok_int ? lds_qf[w][e] : (uint8_t)0u;
    if (ps.ti % MAREC_PER == 0) mafilt_put(line, 7, lok_int ? MAFILT_NONE : 0u);  // the line's "usable" mark
    if (ps.isdown) {
      const bool lok_rad = lds_ok[w][1][e_line] != 0;
      U4 *rline = rec + marec_slot(MADIR_RAD, ps.ti / MAREC_PER, ps.lpk.ndown, ps.lpk.nup);
      mafilt_put(rline, ps.ti % MAREC_PER, lok_rad ? lds_q[w][1][e] : 0u);
      if (ps.ti % MAREC_PER == 0) mafilt_put(rline, 7, lok_rad ? MAFILT_NONE : 0u);
    }
  }
}
__device__ inline double row_shr1(double x);
// The recombination sums of a level (macroatom.cc:147-168: over the levels of the ion below that ionise into it) -- three running sums
// over up to ~60 channels for the 45 levels of the bench's data that have any, none for the other 1522. As a loop of populate_macroatom()
// the lane of such a level walked its list with three dependent gathers per channel while the other 63 lanes of its wave waited
// (k_macroatom at 0.21 lane utilisation). Here a ROW OF 16 LANES per (cell, listed level) reads 16 channels at a time and forms the
// sums with the loop's additions in the loop's order (lane k adds its term to lane k-1's finished sum, as k_cooling_chain does).
__global__ void __launch_bounds__(BLOCK) k_macroatom_recomb(Env env) {
  const int64_t row_id = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 4;
  const int r = threadIdx.x & 15;
  const DevModel &M = env.M;
  const int64_t nrows = fill_count(env) * M.nrecomblevels;
  const bool inrange = row_id < nrows;
  const int c = fill_cell(env, (inrange ? row_id : 0) / M.nrecomblevels);
  const int ul = M.recomb_levels[(inrange ? row_id : 0) % M.nrecomblevels];
  const int ui = M.level_ion[ul];
  const bool valid = inrange && !ma_ion_absent(env, c, ui);  // (an absent ion's records are not populated: tables.h "ABSENT IONS")
  const int ls = M.ion_uniquelevelindexstart[ui > 0 ? ui - 1 : 0];
  const int64_t cb = krow(env, c) * M.nphixstargets_total;
  const double e_cur = eps(M, ul);
  const int j0 = valid ? M.level_recomb_start[ul] : 0, j1 = valid ? M.level_recomb_start[ul + 1] : 0;
  double carry0 = 0., carry1 = 0., carry2 = 0.;
  for (int j = j0; __any(j < j1); j += 16) {
    const bool in = (j + r) < j1;
    double x0 = 0., x1 = 0., x2 = 0.;
    if (in) {
      const int lower = M.recomb_lower[j + r];
      const int t = M.recomb_target[j + r];
      const double e_target = eps(M, ls + lower);
      const double e_trans = e_cur - e_target;
      const int64_t o = cb + M.level_phixstargetstart[ls + lower] + t;
      const double R = env.K.bf_radrecomb[o];
      const double Cc = env.K.bf_colrecomb[o];
      x0 = (R + Cc) * e_target;
      x1 = R * e_trans;
      x2 = Cc * e_trans;
    }
    double a0 = (r == 0) ? carry0 + x0 : x0, a1 = (r == 0) ? carry1 + x1 : x1, a2 = (r == 0) ? carry2 + x2 : x2;
#pragma unroll
    for (int s = 1; s < 16; s++) {
      const double p0 = row_shr1(a0), p1 = row_shr1(a1), p2 = row_shr1(a2);
      if (r == s) {
        a0 = p0 + x0;
        a1 = p1 + x1;
        a2 = p2 + x2;
      }
    }
    // the sums after the row's last channel, broadcast to the row (lanes past the list's end added 0. to them)
    const int src = ((threadIdx.x & 63) | 15) << 2;
    carry0 = __hiloint2double(__builtin_amdgcn_ds_bpermute(src, __double2hiint(a0)), __builtin_amdgcn_ds_bpermute(src, __double2loint(a0)));
    carry1 = __hiloint2double(__builtin_amdgcn_ds_bpermute(src, __double2hiint(a1)), __builtin_amdgcn_ds_bpermute(src, __double2loint(a1)));
    carry2 = __hiloint2double(__builtin_amdgcn_ds_bpermute(src, __double2hiint(a2)), __builtin_amdgcn_ds_bpermute(src, __double2loint(a2)));
  }
  if (valid && r == 0) {
    const LevelPack lpk = M.level_pack[ul];
    double *rates = ma_rates_of(ma_rec_of(env, c, lpk), lpk.ndown, lpk.nup);
    rates[ARTIS_MA_ACTION_INTERNALDOWNLOWER] = carry0;
    rates[ARTIS_MA_ACTION_RADRECOMB] = carry1;
    rates[ARTIS_MA_ACTION_COLRECOMB] = carry2;
  }
}
__global__ void __launch_bounds__(BLOCK) k_macroatom(Env env) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t total = fill_count(env) * env.M.nlevels;
  if (i >= total) return;
  const LevelPack lpk = env.M.level_pack[i % env.M.nlevels];
  if (lpk.rec_off < 0) return;  // (a cold level: filled when a packet reaches it, physics.h ma_slow_fill)
  const int c = fill_cell(env, i / env.M.nlevels);
  if (ma_ion_absent(env, c, env.M.level_ion[i % env.M.nlevels])) {
    // not populated (tables.h "ABSENT IONS"): the marker, at every population of the row; the first visit fills the record (k_slow)
    *ma_rec_of(env, c, lpk) = U4{{MA_MARK_ABSENT, 0u, 0u, 0u}};
    return;
  }
  populate_macroatom<true>(env, c, (int)(i % env.M.nlevels));
}
// The filters of the directions with more transitions than a block of k_matrans holds (DevModel::malongsegs: > MATRANS_BLOCK):
// a wave per (cell, segment) re-forms the running sums 63 transitions (nine filter lines) at a time -- the same terms
// added in the same order, lane k to the finished sum of lane k-1 -- and quantises them with the direction's whole rates,
// which k_matrans has left in the record. (physics.h populate_dirfilter_seq is the sequential form.)
__global__ void __launch_bounds__(BLOCK) k_mafilter_long(Env env) {
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int nseg = env.M.nmalongsegs;
  if (wave >= fill_count(env) * nseg) return;
  const int c = fill_cell(env, wave / nseg);
  const MaLongSeg seg = env.M.malongsegs[wave % nseg];
  const LevelPack lpk = env.M.level_pack[seg.ul];
  if (ma_ion_absent(env, c, env.M.level_ion[seg.ul])) return;  // (the wave: the record is not populated, tables.h "ABSENT IONS")
  U4 *rec = env.K.macache + (krow(env, c) * env.M.nmacache) + lpk.rec_off;
  const double *rates = ma_rates_of(rec, lpk.ndown, lpk.nup);
  const bool down = seg.dir == 0;
  const double whole_int = rates[down ? ARTIS_MA_ACTION_INTERNALDOWNSAME : ARTIS_MA_ACTION_INTERNALUPSAME];
  const double whole_rad = rates[ARTIS_MA_ACTION_RADDEEXC];
  double ca = 0., cb = 0.;
  for (int base = 0; base < seg.n; base += 63) {
    const int ti = base + lane;
    const bool valid = lane < 63 && ti < seg.n;
    double a = 0., b = 0.;
    if (valid) {
      const MaTransTerms t = matrans_terms(env, c, seg.ats0 + ti);
      a = down ? t.v2 : t.v0;
      b = down ? t.v0 : 0.;
    }
    double sa = (lane == 0 ? ca : 0.) + a, sb = (lane == 0 ? cb : 0.) + b;
    for (int k = 1; k < 63; k++) {
      const double pa = wave_shr1(sa), pb = wave_shr1(sb);
      if (lane == k) {
        sa = pa + a;
        sb = pb + b;
      }
    }
    bool ok_int = (whole_int > 0.) && (whole_int <= DBLMAX), ok_rad = (whole_rad > 0.) && (whole_rad <= DBLMAX);
    uint32_t q_int = MAFILT_NONE23, q_rad = MAFILT_NONE;
    if (valid && ti < seg.n - 1) {
      if (ok_int) q_int = mafilt_quant23(sa, whole_int, &ok_int);
      if (ok_rad && down) q_rad = mafilt_quant(sb, whole_rad, &ok_rad);
    }
    const unsigned long long bad_int = __ballot(valid && !ok_int), bad_rad = __ballot(valid && down && !ok_rad);
    if (valid) {
      const unsigned long long mine = line_lanes(lane, ti, seg.n);  // (63 lanes = nine whole lines: lane % 7 == ti % 7)
      const bool lok_int = (bad_int & mine) == 0ull, lok_rad = (bad_rad & mine) == 0ull;
      U4 *line = rec + marec_slot(down ? MADIR_DOWN : MADIR_UP, ti / MAREC_PER, lpk.ndown, lpk.nup);
      mafilt_put23(rec, down ? MADIR_DOWN : MADIR_UP, ti, lpk.ndown, lpk.nup, lok_int ? q_int : 0u);
      if (ti % MAREC_PER == 0) mafilt_put(line, 7, lok_int ? MAFILT_NONE : 0u);
      if (down) {
        U4 *rline = rec + marec_slot(MADIR_RAD, ti / MAREC_PER, lpk.ndown, lpk.nup);
        mafilt_put(rline, ti % MAREC_PER, lok_rad ? q_rad : 0u);
        if (ti % MAREC_PER == 0) mafilt_put(rline, 7, lok_rad ? MAFILT_NONE : 0u);
      }
    }
    const int last = (seg.n - base < 63 ? seg.n - base : 63) - 1;
    ca = __shfl(sa, last);
    cb = __shfl(sb, last);
  }
}
// ---- A cold level's record filled by a WAVE (tables.h "ON-DEMAND RECORDS"; physics.h ma_fill_record is the sequential form, which one lane of
// the slow-path kernel ran in the first version: 585 ms of a 6.5 s step with the w7big data, most of the 3.3 s of k_slow with cd23like). The
// transitions' terms -- the expensive part: rate coefficients with exp() and divisions -- are evaluated by 63 lanes side by side; the running
// sums are formed in the sequential loop's order (lane j ends with carry + t_0 + ... + t_j, added left to right); each lane quantises its own
// entry, a filter line's "usable" mark is a vote of its lanes (as in k_mafilter_long); lane 0 writes the rates and runs the bound-free part
// and the action filter (populate_macroatom). Same terms, same additions in the same order: the same bits (GPU test: the records a run
// left in the pool against populate_dirfilter_seq, artis_amd_debug_cellcache()).
__device__ inline double wave_prefix_inorder(double t, double carry, int n, int lane) {
  double acc = carry;
  for (int k = 0; k < n; k++) {
    const double x = wave_bcast(t, k);
    if (lane >= k) acc += x;
  }
  return acc;
}
// ... NS running sums at once, through LDS (round 6): the lanes leave their terms in the wave's own rows, lane j < NS adds row j up from left to
// right -- the same additions in the same order, so the same bits -- and every lane reads its sums back. As broadcasts and masked additions the
// three sums of a block of 63 transitions were ~950 wave instructions; this is 63 dependent additions by three lanes side by side (the fills
// of the 4e5-line set: 2.1 s of its 17 s step).
constexpr int PREFIX_ROWS = 3;
// the wave's rows (one set for all instantiations: 12 KB per workgroup of BLOCK threads)
__device__ inline double (*prefix_rows(bool out))[64] {
  __shared__ double rows_in[BLOCK / 64][PREFIX_ROWS][64];
  __shared__ double rows_out[BLOCK / 64][PREFIX_ROWS][64];
  const int w = (int)(threadIdx.x >> 6) % (BLOCK / 64);
  return out ? rows_out[w] : rows_in[w];
}
template <int NS>
__device__ inline void wave_prefix_inorder_n(const double (&t)[NS], const double (&carry)[NS], int n, int lane, double (&out)[NS]) {
  static_assert(NS <= PREFIX_ROWS, "rows");
  double(*rin)[64] = prefix_rows(false);
  double(*rout)[64] = prefix_rows(true);
#pragma unroll
  for (int j = 0; j < NS; j++) rin[j][lane] = t[j];
  __threadfence_block();  // (lanes of one wave exchange data through LDS: in order, but the compiler must not move the accesses)
  if (lane < NS) {
    double acc = 0.;
#pragma unroll
    for (int j = 0; j < NS; j++) acc = (lane == j) ? carry[j] : acc;
    const double *in = rin[lane];
    double *o = rout[lane];
    for (int k = 0; k < n; k++) {
      acc += in[k];
      o[k] = acc;
    }
  }
  __threadfence_block();
  const int k = (lane < n) ? lane : n - 1;  // (a lane past the block's last transition holds the block's total, as wave_prefix_inorder() gives it)
#pragma unroll
  for (int j = 0; j < NS; j++) out[j] = rout[j][k];
  __threadfence_block();  // (the next call writes the rows again)
}
// the entries of one block (lanes 0..62 = transitions base .. base + 62 of a direction of n) into the record: internal filter from s_int,
// radiative filter (downward only) from s_rad
__device__ inline void wave_put_dirfilters(U4 *rec, const LevelPack &lpk, bool down, int n, int ti, bool valid, double s_int, double s_rad,
                                           double whole_int, double whole_rad, int lane) {
  bool ok_int = (whole_int > 0.) && (whole_int <= DBLMAX), ok_rad = (whole_rad > 0.) && (whole_rad <= DBLMAX);
  uint32_t q_int = MAFILT_NONE23, q_rad = MAFILT_NONE;
  if (valid && ti < n - 1) {
    if (ok_int) q_int = mafilt_quant23(s_int, whole_int, &ok_int);
    if (ok_rad && down) q_rad = mafilt_quant(s_rad, whole_rad, &ok_rad);
  }
  const unsigned long long bad_int = __ballot(valid && !ok_int), bad_rad = __ballot(valid && down && !ok_rad);
  if (valid) {
    const unsigned long long mine = line_lanes(lane, ti, n);
    const bool lok_int = (bad_int & mine) == 0ull, lok_rad = (bad_rad & mine) == 0ull;
    U4 *line = rec + marec_slot(down ? MADIR_DOWN : MADIR_UP, ti / MAREC_PER, lpk.ndown, lpk.nup);
    mafilt_put23(rec, down ? MADIR_DOWN : MADIR_UP, ti, lpk.ndown, lpk.nup, lok_int ? q_int : 0u);
    if (ti % MAREC_PER == 0) mafilt_put(line, 7, lok_int ? MAFILT_NONE : 0u);
    if (down) {
      U4 *rline = rec + marec_slot(MADIR_RAD, ti / MAREC_PER, lpk.ndown, lpk.nup);
      mafilt_put(rline, ti % MAREC_PER, lok_rad ? q_rad : 0u);
      if (ti % MAREC_PER == 0) mafilt_put(rline, 7, lok_rad ? MAFILT_NONE : 0u);
    }
  }
}
// STATIC_SLOT (tables.h "ABSENT IONS"): the record is a static one the population left out. Its action filter (slot 0) holds the marker until
// lane 0 stores the filter as the record's LAST write, and its cooling filter -- which the population wrote like every level's (k_collexc_filter),
// and which k-packets read without asking for the record -- is left as it stands.
template <bool STATIC_SLOT = false>
__device__ inline void ma_fill_record_wave(const Env &env, int c, int ul) {
  const DevModel &M = env.M;
  const int lane = (int)(threadIdx.x & 63);
  const LevelPack lpk = M.level_pack[ul];
  U4 *rec = ma_rec_of(env, c, lpk);
  const int nd = lpk.ndown, nu = lpk.nup;
  {  // populate_mainit_at(): every filter entry "never counted", the rates zero
    const int nfilt = marec_rates_slot(nd, nu), nfine0 = marec_fine_slot0(nd, nu), nrec = marec_slots(nd, nu);
    const int ntot = ((nrec + MAREC_ALIGN - 1) / MAREC_ALIGN) * MAREC_ALIGN;
    const int ncool0 = marec_slot(MADIR_COOL, 0, nd, nu);
    const uint32_t none2 = MAFILT_NONE | (MAFILT_NONE << 16);
    for (int i = lane; i < ntot; i += 64) {
      if (STATIC_SLOT && (i == 0 || (i >= ncool0 && i < nfilt))) continue;
      rec[i] = (i < nfilt) ? U4{{none2, none2, none2, none2}} : ((i >= nfine0 && i < nrec) ? U4{{~0u, ~0u, ~0u, ~0u}} : U4{{0u, 0u, 0u, 0u}});
    }
  }
  __threadfence_block();  // (other lanes write into these slots below)
  // ---- downward: rates (radiative, collisional de-excitation, internal down), then the internal-down and radiative filters
  double w_rad = 0., w_col = 0., w_down = 0.;
  double b0_rad = 0., b0_down = 0.;  // block 0's running sums, kept for a direction of one block (no second evaluation of its terms)
  for (int base = 0; base < nd; base += 63) {
    const int nb = (nd - base < 63) ? nd - base : 63;
    const bool valid = lane < nb;
    double v0 = 0., v1 = 0., v2 = 0.;
    if (valid) {
      const MaTransTerms t = matrans_terms(env, c, lpk.alltrans_startdown + base + lane);
      v0 = t.v0; v1 = t.v1; v2 = t.v2;
    }
    double ss[3];
    wave_prefix_inorder_n<3>({v0, v1, v2}, {w_rad, w_col, w_down}, nb, lane, ss);
    const double s0 = ss[0], s1 = ss[1], s2 = ss[2];
    if (base == 0) { b0_rad = s0; b0_down = s2; }
    w_rad = wave_bcast(s0, nb - 1);
    w_col = wave_bcast(s1, nb - 1);
    w_down = wave_bcast(s2, nb - 1);
  }
  if (nd > 0 && nd <= 63) {
    wave_put_dirfilters(rec, lpk, true, nd, lane, lane < nd, b0_down, b0_rad, w_down, w_rad, lane);
  } else {
    double c_rad = 0., c_down = 0.;
    for (int base = 0; base < nd; base += 63) {
      const int nb = (nd - base < 63) ? nd - base : 63;
      const bool valid = lane < nb;
      double v0 = 0., v2 = 0.;
      if (valid) {
        const MaTransTerms t = matrans_terms(env, c, lpk.alltrans_startdown + base + lane);
        v0 = t.v0; v2 = t.v2;
      }
      double ss[2];
      wave_prefix_inorder_n<2>({v0, v2}, {c_rad, c_down}, nb, lane, ss);
      const double s0 = ss[0], s2 = ss[1];
      wave_put_dirfilters(rec, lpk, true, nd, base + lane, valid, s2, s0, w_down, w_rad, lane);
      c_rad = wave_bcast(s0, nb - 1);
      c_down = wave_bcast(s2, nb - 1);
    }
  }
  // ---- upward: the internal-up rate and filter, and the level's collisional-excitation cooling filter (running sums from the
  // cooling list's value before the level; populate_coolfilter_level_seq)
  const int hi_i = M.level_coolhi[ul];
  const double *cool = env.K.cooling_contrib + (krow(env, c) * M.ncoolingterms);
  const double c_hi = (nu > 0 && hi_i >= 0) ? cool[hi_i] : 0.;
  const double c_lo = (nu > 0 && hi_i > M.ion_coolingoffset[M.level_ion[ul]]) ? cool[hi_i - 1] : 0.;
  const double span = c_hi - c_lo;
  double w_up = 0.;
  double b0_up = 0., b0_kt = 0.;
  for (int base = 0; base < nu; base += 63) {
    const int nb = (nu - base < 63) ? nu - base : 63;
    double v0 = 0., kt = 0.;
    if (lane < nb) {
      const MaTransTerms t = matrans_terms(env, c, lpk.alltrans_startdown + nd + base + lane);
      v0 = t.v0; kt = t.kterm;
    }
    double ss[1];
    wave_prefix_inorder_n<1>({v0}, {w_up}, nb, lane, ss);
    const double s0 = ss[0];
    if (base == 0) { b0_up = s0; b0_kt = kt; }
    w_up = wave_bcast(s0, nb - 1);
  }
  {
    double c_up = 0., c_cool = c_lo;
    for (int base = 0; base < nu; base += 63) {
      const int nb = (nu - base < 63) ? nu - base : 63;
      const bool valid = lane < nb;
      const int ti = base + lane;
      double v0 = 0., kt = b0_kt;
      if (valid && nu > 63) {  // (a direction of one block keeps its terms from the pass above)
        const MaTransTerms t = matrans_terms(env, c, lpk.alltrans_startdown + nd + base + lane);
        v0 = t.v0; kt = t.kterm;
      }
      // (the internal-up sums again -- a direction of one block keeps them from the pass above -- and the cooling terms' sums from the list's
      // value before the level, side by side)
      double ss[2];
      wave_prefix_inorder_n<2>({v0, kt}, {c_up, c_cool}, nb, lane, ss);
      const double s0 = (nu <= 63) ? b0_up : ss[0];
      wave_put_dirfilters(rec, lpk, false, nu, ti, valid, s0, 0., w_up, 0., lane);
      c_up = wave_bcast(s0, nb - 1);
      if (!STATIC_SLOT && hi_i >= 0) {
        const double sk = ss[1];
        bool ok = (span > 0.) && (span <= DBLMAX);
        uint32_t q = MAFILT_NONE;
        if (valid && ti < nu - 1 && ok) q = mafilt_quant(sk - c_lo, span, &ok);
        const unsigned long long bad = __ballot(valid && !ok);
        if (valid) {
          const bool lok = (bad & line_lanes(lane, ti, nu)) == 0ull;
          U4 *line = rec + marec_slot(MADIR_COOL, ti / MAREC_PER, nd, nu);
          if (lok) {
            mafilt_put(line, ti % MAREC_PER, q);
          } else if (ti % MAREC_PER == 0) {
            *line = U4{{0u, 0u, 0u, 0u}};  // (populate_coolfilter_line: a line that is not usable is all zero, its mark too)
          }
        }
        c_cool = wave_bcast(sk, nb - 1);
      }
    }
  }
  __threadfence_block();
  if (lane == 0) {
    double *rates = ma_rates_of(rec, nd, nu);
    rates[ARTIS_MA_ACTION_RADDEEXC] = w_rad;
    rates[ARTIS_MA_ACTION_COLDEEXC] = w_col;
    rates[ARTIS_MA_ACTION_INTERNALDOWNSAME] = w_down;
    rates[ARTIS_MA_ACTION_INTERNALUPSAME] = w_up;
    populate_macroatom<false, STATIC_SLOT>(env, c, ul);  // the bound-free channels and the action filter (a static slot's: after a release)
  }
}
// every lane of the wave whose packet waits for a record it has claimed (physics.h ma_slow_fill_claim) gets it filled, lane by lane
template <bool STATIC_SLOT = false>
__device__ inline void ma_fill_wave(const Env &env, bool mine, int c, int ul) {
  unsigned long long m = __ballot(mine);
  while (m != 0) {
    const int src = __ffsll((long long)m) - 1;
    ma_fill_record_wave<STATIC_SLOT>(env, __builtin_amdgcn_readlane(c, src), __builtin_amdgcn_readlane(ul, src));
    m &= m - 1;
  }
}
// ABSENT IONS (tables.h): the packet waits (PEND_MA_FILL) in a level with a STATIC record that the population left out. The lane claims the record
// with a compare-and-swap on the marker word (absent -> being filled); true: the wave is to fill it (ma_fill_wave<true>). A lane that loses the
// claim -- another lane won it, in this launch or an earlier one -- goes back to its list: the record is complete when this launch ends.
__device__ inline bool ma_static_fill_claim(const Env &env, const Pkt &p, int *c_out, int *ul_out) {
  const DevModel &M = env.M;
  const int c = M.propcell_nonemptymgi[p.cellindex];
  const int ul = M.ion_uniquelevelindexstart[uion(M, p.ma_element, p.ma_ion)] + p.ma_level;
  const LevelPack lpk = M.level_pack[ul];
  if (lpk.rec_off < 0) return false;
  uint32_t *w0 = (uint32_t *)(env.K.macache + (krow(env, c) * M.nmacache) + lpk.rec_off);
  if (__hip_atomic_load(w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != MA_MARK_ABSENT) return false;
  if (atomicCAS(w0, MA_MARK_ABSENT, MA_MARK_FILLING) != MA_MARK_ABSENT) return false;
  atomicAdd(env.ma_absent_counts + 1, 1ull);
  *c_out = c;
  *ul_out = ul;
  return true;
}
// test / debug view of one cell's records (artis_amd_debug_cellcache): a thread per level
__global__ void __launch_bounds__(BLOCK) k_debug_macache(Env env, int c, double *maprocessrates, double *matrans, int32_t *bad) {
  const int ul = blockIdx.x * BLOCK + threadIdx.x;
  if (ul >= env.M.nlevels) return;
  if (ma_resolve(env, c, env.M.level_pack[ul].rec_off) == MA_REC_NONE) return;  // (a cold level no packet has reached in this cell: no record)
  // a static record the population left out (tables.h "ABSENT IONS") is filled before it is read: the sequential forms, as for a cold level
  if (env.M.level_pack[ul].rec_off >= 0 && ma_mark_unpopulated(ma_rec_of(env, c, env.M.level_pack[ul])->w[0])) ma_fill_record(env, c, ul);
  const int b = debug_level_record(env, c, ul, maprocessrates, matrans);
  if (b != 0) atomicAdd(bad, b);
}
// before a fill: no cold level of the cells to be filled has a record (tables.h "ON-DEMAND RECORDS"; the pool itself is emptied by populate_tile())
__global__ void __launch_bounds__(BLOCK) k_ma_reset(Env env) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int ncold = env.M.ncold;
  if (i >= fill_count(env) * ncold) return;
  const int c = fill_cell(env, i / ncold);
  env.K.ma_rowtab[(krow(env, c) * ncold) + (i % ncold)] = -1;
}
// the static part of every record of every resident row, once per engine: filter entries "never counted", lines usable
__global__ void __launch_bounds__(BLOCK) k_mainit(Env env, int64_t nrows) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= nrows * env.M.nlevels) return;
  populate_mainit(env, i / env.M.nlevels, (int)(i % env.M.nlevels));
}
// The cooling list of a (cell, ion) is one running sum over hundreds of terms (kpkt.cc:57-190): a free-free term, the
// collisional-excitation terms k_matrans left in the population's scratch rows (most of them), and the bound-free tail. Three kernels:
// head and tail with a lane per (cell, ion) -- 64 chains side by side, each short -- and the long middle with a ROW OF
// 16 LANES per (cell, ion): it reads 16 terms (one cache line) at a time, forms the running sum with the sequential
// additions of the reference's loop (lane k adds its term to lane k-1's finished sum: DPP row shifts, same order, same
// bits), writes it back and drops the level totals into the cooling list through the static slot table. (A lane per
// chain walked the terms with strided 8-byte accesses: 35 ms per step for the three parts, now 15.) The running sum
// travels between the kernels in ion_cooling_C.
__global__ void __launch_bounds__(BLOCK) k_cooling_head(Env env) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t total = fill_count(env) * env.M.nions;
  if (i >= total) return;
  const int c = fill_cell(env, i / env.M.nions);
  const int ui = (int)(i % env.M.nions);
  int k = 0;
  env.K.ion_cooling_C[(krow(env, c) * env.M.nions) + ui] = cooling_ion_head(env, c, ui, &k);
}
// the value of the lane below within a row of 16 lanes (the row's first lane: 0)
__device__ inline double row_shr1(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x111 /* row_shr:1 */, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// Four chains per wave, one per row of 16 lanes: a row reads 16 terms (one 128-byte line) at a time and needs 15 serial
// steps for them; four independent chains keep the wave's issue slots four times as busy as one chain of 64 would.
__global__ void __launch_bounds__(BLOCK) k_cooling_chain(Env env) {
  const int64_t row_id = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 4;
  const int r = threadIdx.x & 15;
  const DevModel &M = env.M;
  const int64_t nchains = fill_count(env) * M.nions;
  const bool valid = row_id < nchains;
  const int c = fill_cell(env, (valid ? row_id : 0) / M.nions);
  const int ui = (int)((valid ? row_id : 0) % M.nions);
  const int start = M.ion_uniquelevelindexstart[ui];
  const int nlevels = M.ion_nlevels[ui];
  const int j0 = (valid && nlevels > 0) ? M.level_upcum_start[start] : 0;
  const int j1 = (valid && nlevels > 0) ? M.level_upcum_start[start + nlevels - 1] + M.level_nuptrans[start + nlevels - 1] : 0;
  double carry = valid ? env.K.ion_cooling_C[(krow(env, c) * M.nions) + ui] : 0.;
  double *upcum = env.collexc_terms + (((valid ? row_id : 0) / M.nions) * M.nupcum);  // the cell's row of the population's scratch
  double *cool = env.K.cooling_contrib + (krow(env, c) * M.ncoolingterms);
  for (int j = j0; __any(j < j1); j += 16) {  // rows with shorter chains idle through the longer ones' chunks
    const bool in = (j + r) < j1;
    const double x = in ? upcum[j + r] : 0.;
    double acc = (r == 0) ? carry + x : x;
#pragma unroll
    for (int s = 1; s < 16; s++) {
      const double prev = row_shr1(acc);  // lane s-1 of the row holds its finished sum
      if (r == s) acc = prev + x;
    }
    if (in) {
      upcum[j + r] = acc;
      const int slot = M.upcum_coolslot[j + r];
      if (slot >= 0) cool[slot] = acc;
    }
    // the sum after the row's last term, broadcast to the row (lanes past the end added 0. to it: x + 0. == x exactly)
    const int src = ((threadIdx.x & 63) | 15) << 2;
    carry = __hiloint2double(__builtin_amdgcn_ds_bpermute(src, __double2hiint(acc)), __builtin_amdgcn_ds_bpermute(src, __double2loint(acc)));
  }
  if (valid && r == 0 && j1 > j0) env.K.ion_cooling_C[(krow(env, c) * M.nions) + ui] = carry;
}
// the cooling filters of the levels' records from the running sums the chain left in the scratch rows: a thread per (cell, line)
__global__ void __launch_bounds__(BLOCK) k_collexc_filter(Env env) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t per = env.M.ncoollines;
  if (i >= fill_count(env) * per) return;
  const int64_t kf = i / per;
  populate_coolfilter_line(env, fill_cell(env, kf), (int)(i % per), env.collexc_terms + (kf * env.M.nupcum));
}
// The bound-free tail of an ion's cooling list (kpkt.cc:122-190: a collisional-ionisation term and then a bound-free term per (ionising
// level, target), ~120 entries, each behind three or four dependent gathers): a lane per (cell, ion) walked it serially (11 ms per step).
// Round 4: a ROW OF 16 LANES per (cell, ion), like k_cooling_chain -- every lane forms the term of one entry (what the entry is it reads
// from the cooling list's own static tables, checked against the loop order when the engine is created), the running sum is formed with the
// loop's additions in the loop's order (DPP row shifts) and written back 16 entries = one 128-byte line at a time.
// physics.h cooling_ion_tail() is the sequential form (test emulation).
__global__ void __launch_bounds__(BLOCK) k_cooling_tail(Env env) {
  const int64_t row_id = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 4;
  const int r = threadIdx.x & 15;
  const DevModel &M = env.M;
  const int64_t nrows = fill_count(env) * M.nions;
  const bool valid = row_id < nrows;
  const int c = fill_cell(env, (valid ? row_id : 0) / M.nions);
  const int ui = (int)((valid ? row_id : 0) % M.nions);
  const int element = M.ion_element[ui];
  const int ion = ui - M.elem_uniqueionindexstart[element];
  const bool has = valid && ion < (M.elem_nions[element] - 1) && M.nbfcontinua > 0;
  const double *pops = env.K.levelpops + (krow(env, c) * M.nlevels);
  const int ionstart = M.ion_coolingoffset[ui];
  double *contribs = env.K.cooling_contrib + (krow(env, c) * M.ncoolingterms) + ionstart;
  const float cnne = clumpednne(env.C, c);
  const float T_e = env.C.Te[c];
  const int start = M.ion_uniquelevelindexstart[ui];
  const int ustart = has ? M.ion_uniquelevelindexstart[ui + 1] : 0;
  const double nnupperion = has ? nnion(env, c, element, ion + 1) : 0.;
  const int k0 = has ? M.ion_cooltail_start[ui] : 0, k1 = has ? M.ion_ncoolingterms[ui] : 0;
  double carry = valid ? env.K.ion_cooling_C[(krow(env, c) * M.nions) + ui] : 0.;
  for (int j = k0; __any(j < k1); j += 16) {
    const bool in = (j + r) < k1;
    double x = 0.;
    if (in) {
      const int i = ionstart + j + r;
      const int level = M.coolinglist_level[i];
      const int t = M.coolinglist_phixstargetindex[i];
      const int ul = start + level;
      const int64_t o = (krow(env, c) * M.nphixstargets_total) + M.level_phixstargetstart[ul];
      if (M.coolinglist_type[i] == ARTIS_COOLING_COLLION) {
        const double e_trans = eps(M, ustart + phixs_upperlevel(M, ul, t)) - eps(M, ul);
        x = pops[ul] * env.K.bf_colion[o + t] * e_trans;
      } else {
        double pop;
#if ARTIS_OPT_BFCOOLING_USELEVELPOPNOTIONPOP
        pop = pops[ustart + phixs_upperlevel(M, ul, t)];
#else
        const int nt = M.level_nphixstargets[ul];
        if (nt == 1) {
          pop = nnupperion;
        } else {
          double E_min = DBLMAX;
          for (int tt = 0; tt < nt; tt++) E_min = dmin(E_min, eps(M, ustart + phixs_upperlevel(M, ul, tt)));
          double wsum = 0.;
          for (int tt = 0; tt < nt; tt++) {
            const int up = phixs_upperlevel(M, ul, tt);
            wsum += statw(M, ustart + up) * exp(-(eps(M, ustart + up) - E_min) / KB / T_e);
          }
          const int up = phixs_upperlevel(M, ul, t);
          const double w = statw(M, ustart + up) * exp(-(eps(M, ustart + up) - E_min) / KB / T_e);
          pop = nnupperion * w / wsum;
        }
#endif
        x = env.K.bf_cooling[o + t] * pop * cnne;
      }
    }
    double acc = (r == 0) ? carry + x : x;
#pragma unroll
    for (int s = 1; s < 16; s++) {
      const double prev = row_shr1(acc);
      if (r == s) acc = prev + x;
    }
    if (in) contribs[j + r] = acc;
    const int src = ((threadIdx.x & 63) | 15) << 2;
    carry = __hiloint2double(__builtin_amdgcn_ds_bpermute(src, __double2hiint(acc)), __builtin_amdgcn_ds_bpermute(src, __double2loint(acc)));
  }
  if (has && r == 0) env.K.ion_cooling_C[(krow(env, c) * M.nions) + ui] = carry;
}
__global__ void __launch_bounds__(BLOCK) k_cooling_prefix(Env env) {
  const int64_t kf = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (kf >= fill_count(env)) return;
  const int c = fill_cell(env, kf);
  populate_cooling_prefix(env, c);
}
// the guides of the two cumulative lists a k-packet step draws from (tables.h "COOLING GUIDES"): a thread per entry
__global__ void __launch_bounds__(BLOCK) k_cool_guide(Env env) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t total = fill_count(env) * env.M.nguide;
  if (i >= total) return;
  populate_cool_guide(env, fill_cell(env, i / env.M.nguide), (int)(i % env.M.nguide));
}
