// stage_propagate.h -- artis_amd_update_packets_device: the host's side of propagating the resident packets through one timestep.
// Sweeps over the cell-cache tiles (one tile, one sweep when the whole cache is resident): list the packets that sit in the tile, fill the
// tile's cache if any do, advance them until they leave the tile or are done; repeat until a sweep finds no packet left to advance.
#pragma once
namespace {
// a step's return code: anything but ARTIS_OK ends the call
#define STEP(expr)                     \
  do {                                 \
    const int _rc = (expr);            \
    if (_rc != ARTIS_OK) return _rc;   \
  } while (0)
template <int N>
using Int = std::integral_constant<int, N>;  // a template argument chosen at run time, handed to the generic lambda that makes the launch
// counting sort of list[0..n) by its entries' keys into e->d_sorted; *out = the list to launch on
// max_per_cell: a list with more entries per cell than this stays in the order it was appended in. A cell-sorted list puts every lane that is running on
// an XCD into the same few cells when the cells are few and full, and their estimator atomics then hit the same few addresses at the same time
// (device-wide atomics on one address are serialised in memory: 20^3 cells, 1e7 packets: k_thermal 907 ms sorted, 725 ms unsorted), while the locality
// the sort buys matters less because fewer cells' tables compete for the caches. Models with so few cells that the kernels accumulate their per-cell
// estimators in LDS (Env::cellest_lds) have no such atomics and are always sorted (6^3 cells: 494 ms sorted, 593 unsorted).
// into: where the sorted list goes, if not e->d_sorted
int sort_by_key(artis_amd_engine *e, hipStream_t s, const int32_t *list, const int32_t *keys, int32_t n, const int32_t **out, int nbins,
                int64_t ncells, int max_per_cell, int32_t nkeys_given = 0, int32_t *into = nullptr) {
  *out = list;
  if (!e->sort_lists || n < 2 * BLOCK) return ARTIS_OK;
  if ((int64_t)n > (int64_t)max_per_cell * (ncells > 0 ? ncells : 1)) return ARTIS_OK;
  if (into == nullptr) into = e->d_sorted;
  STEP(sort_list(e, s, list, keys, n, nkeys_given > 0 ? (int64_t)nkeys_given : (int64_t)e->Mh.ngrid * nbins, into));
  *out = into;
  return ARTIS_OK;
}
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
// the estimator updates the propagation launch before it recorded (the cells' cache rows are still resident)
void launch_bfest_dense(artis_amd_engine *e, const Env &env, hipStream_t s) {
  const bool lds = e->dense_cont_lds && e->Mh.nbfcontinua <= CONT_LDS_MAX;
  e->last.est_forms |= (lds ? ARTIS_AMD_EST_BF_DENSE_CONTLDS : ARTIS_AMD_EST_BF_DENSE_HBM) |
                       (e->dense_lpr == 64 ? ARTIS_AMD_EST_BF_LPR64 : (e->dense_lpr == 16 ? ARTIS_AMD_EST_BF_LPR16 : ARTIS_AMD_EST_BF_LPR32));
  auto launch = [&](auto lpr) {
    if (lds)
      hipLaunchKernelGGL((k_bfest_dense<true, DENSE_TB, decltype(lpr)::value>), dim3(e->ncu * ARTIS_DENSE_WGS), dim3(DENSE_TB), 0, s, env);
    else
      hipLaunchKernelGGL((k_bfest_dense<false, BLOCK, decltype(lpr)::value>), dim3(e->ncu * 8), dim3(BLOCK), 0, s, env);
  };
  if (e->dense_lpr == 64)
    launch(Int<64>{});
  else if (e->dense_lpr == 16)
    launch(Int<16>{});
  else
    launch(Int<32>{});
}
#endif
// the text of a kernel's error flag. Flag 46 reads differently after a launch (the pool cannot hold one record) and at the call's end.
std::string errflag_text(int32_t flag, bool at_call_end) {
  if (flag == 47) return "k_late: a wave waited in vain for its turn to publish queue entries (error flag 47): a fault of the kernel's queue protocol";
  if (flag != 46) return "a kernel raised error flag " + std::to_string(flag) + " (an assert_always of the reference would have fired)";
  return std::string(at_call_end ? "a cell's pool of on-demand macro-atom records is used up"
                                 : "the pool of on-demand macro-atom records cannot hold a single record of this atomic data") +
         " (error flag 46): raise ARTIS_AMD_MA_POOLFRAC (or ARTIS_AMD_MA_HOTFRAC)";
}
// f(std::true_type{}) or f(std::false_type{}): a run-time flag as a template argument of the launch f makes
template <class F>
void with_flag(bool flag, F &&f) {
  flag ? f(std::true_type{}) : f(std::false_type{});
}
// the state of one artis_amd_update_packets_device call; its members are the steps, the entry point at the end is the loop over sweeps, tiles and visits
struct PropRun {
  using clk = std::chrono::steady_clock;
  static double since(clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); }
  artis_amd_engine *const e;  // (an aggregate: PropRun run{e, s})
  const hipStream_t s;
  Env env = make_env(e);
  int cur[NEXT_NKINDS] = {};        // which of the two buffers is the current list of each kind
  int32_t cnt[2 * NEXT_NKINDS] = {};  // host copy of the device counters
  bool pool_reset_due = false, first_pass = true;
  const int r_nubins = e->sort_nu ? SORT_NUBINS : 1;  // frequency bins in the keys of the r-packet list
  // cell groups of the frequency-major keys: the ONE number both the keys (Lists::numajor) and the sort's key count are made of
  const int32_t r_ngroups = (e->sort_cellshift > 0) ? ((e->Mh.ngrid >> e->sort_cellshift) + 1) : e->Mh.ngrid;
  const bool adaptive = e->cc.tile_adapt && e->cc.ntiles > 1;
  int64_t guard = 0;
  // (ARTIS_AMD_TRACE: where the host's time of the call goes -- waiting for the stream, submitting sorts, submitting launches)
  double wall_sync = 0., wall_sort = 0., wall_launch = 0.;
  clk::time_point t_launch;         // when run_kind() began to submit its launch
  std::vector<int32_t> want;        // the cells prepare_visit() asks for
  int64_t listed = 0;               // packets the current visit began with
  int64_t visit_launches = 0;       // split-kernel launches of this visit (a visit parks its tail only after it has advanced its packets)
  Lists lists_for(int self_kind) const {
    Lists L;
    for (int k = 0; k < NEXT_NKINDS; k++) {
      L.lst[k] = e->d_lists[k][cur[k]];
      L.key[k] = e->d_keys[k][cur[k]];
    }
    L.counts = e->d_count;
    L.self_kind = self_kind;
    L.self_list = self_kind > 0 ? e->d_lists[self_kind][1 - cur[self_kind]] : nullptr;
    L.self_key = self_kind > 0 ? e->d_keys[self_kind][1 - cur[self_kind]] : nullptr;
    L.self_count = e->d_count + NEXT_NKINDS;  // one alternate counter: only one kernel runs at a time
    L.kpkt_slot = NEXT_MA;  // k-packets travel in the thermal list
    L.nubins = r_nubins;
    L.numajor = e->sort_numajor ? r_ngroups : 0;
    L.cellshift = e->sort_cellshift;
    L.mabins = e->ma_bins;
    return L;
  }
  int read_counts() {
    // (one copy into pinned memory: counters and error flag are neighbours. Two copies into the stack -- pageable, staged by the runtime -- were a
    // measurable share of the ~90 ms a headline step spends outside its kernels)
    const clk::time_point t_sync = clk::now();
    HIP_TRY(hipMemcpyAsync(e->h_counts, e->d_count, sizeof(int32_t) * (2 * NEXT_NKINDS + 2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    wall_sync += since(t_sync);
    std::memcpy(cnt, e->h_counts, sizeof(int32_t) * 2 * NEXT_NKINDS);
    const int32_t errflag = e->h_counts[2 * NEXT_NKINDS];
    HIP_TRY(hipGetLastError());
    if (errflag != 0) {
      g_last_error = errflag_text(errflag, false);
      (void)hipMemsetAsync(e->d_err, 0, sizeof(int32_t), s);
      return ARTIS_ERR_NOTCONVERGED;
    }
    if (cnt[2 * NEXT_NKINDS - 1] != 0) {  // a lane found the pool of on-demand records used up (Env::ma_pool_full)
      pool_reset_due = true;
      HIP_TRY(hipMemsetAsync(e->d_count + (2 * NEXT_NKINDS - 1), 0, sizeof(int32_t), s));
    }
    return ARTIS_OK;
  }
  // The pool of on-demand records used up: the packets that wait for a record sit on the slow-path list (PEND_MA_FILL). Before that list's next
  // launch -- after the thermal kernel has walked on with the records the last one filled -- the pool is emptied: every cold level of the resident
  // cells is without a record again and is filled when next needed, exactly as after a tile's refill. Costs fills, never an answer.
  int reset_pool_if_due() {
    if (!pool_reset_due || e->Mh.ncold <= 0) return ARTIS_OK;
    pool_reset_due = false;
    HIP_TRY(hipMemsetAsync(e->K.ma_rowtab, 0xFF, sizeof(int32_t) * (size_t)(e->cc.res.tile_cells * (int64_t)e->Mh.ncold), s));  // (every row: k_ma_reset)
    HIP_TRY(hipMemsetAsync(e->K.ma_pool_used, 0, sizeof(uint32_t), s));
    e->last.pool_resets++;
    if (e->trace) fprintf(stderr, "[artis_amd] the pool of on-demand records was used up: emptied (%lld)\n", (long long)e->last.pool_resets);
    return ARTIS_OK;
  }
  // Before a visit: the cache rows its packets need. Tiled: where do the packets wait? The cells in which most of them do are made resident
  // (choose_cells(): a window or a set of blocks of cells, or -- few packets -- the very cells); cells that are resident already keep their rows,
  // the others are filled; *nothing_left is set where no packet waits anywhere. Untiled: the whole cache, if the cell state has changed since its last fill.
  int prepare_visit(int tile, bool *nothing_left) {
    const int64_t ncell_all = e->Mh.npts_nonempty;
    if (e->cc.ntiles > 1) {
      env = make_env(e);
      HIP_TRY(hipMemsetAsync(e->cc.d_waiting, 0, sizeof(int32_t) * (size_t)(ncell_all + 1), s));
      hipLaunchKernelGGL(k_count_waiting, dim3(nblocks(e->npackets)), dim3(BLOCK), 0, s, env, e->cc.d_waiting, e->cc.d_waiting + ncell_all);
      HIP_TRY(hipMemcpyAsync(e->cc.h_waiting.data(), e->cc.d_waiting, sizeof(int32_t) * (size_t)(ncell_all + 1), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      int64_t total = 0;
      for (int64_t c = 0; c < ncell_all; c++) total += e->cc.h_waiting[(size_t)c];
      if (total == 0 && e->cc.h_waiting[(size_t)ncell_all] == 0) {
        *nothing_left = true;
        return ARTIS_OK;
      }
      int64_t holds = 0, nfilled = 0;
      bool sparse = false;
      choose_cells(e, e->cc.h_waiting, want, &holds, &sparse, adaptive ? -1 : (int64_t)tile * e->cc.res.tile_cells);
      if (holds == 0) want.clear();  // (no packet waits for a row of these cells: the visit is for the packets that need none, if any)
      if (e->trace)
        fprintf(stderr, "[artis_amd] visit %lld: %lld packets wait in cells, %d need no row; %zu cells chosen%s hold %lld\n", (long long)e->last_visits,
                (long long)total, e->cc.h_waiting[(size_t)ncell_all], want.size(), sparse ? " (sparse)" : "", (long long)holds);
      HIP_TRY(hipEventRecord(e->ev2, s));
      STEP(make_resident(e, want, s, &nfilled));
      if (nfilled > 0) {
        HIP_TRY(hipEventRecord(e->ev3, s));
        HIP_TRY(hipEventSynchronize(e->ev3));
        float fms = 0.f;
        HIP_TRY(hipEventElapsedTime(&fms, e->ev2, e->ev3));
        e->last.fill_ms += fms;
        e->last.tile_fills++;
        e->last.cells_filled += nfilled;
        if (sparse) e->last.sparse_fills++;
      }
    } else if (e->cc.tile_valid_lo != 0) {
      STEP(populate_tile(e, s));
    }
    env = make_env(e);
    return ARTIS_OK;
  }
  // the packets that sit in resident cells (and those that need no row) onto the lists of their kinds; cnt[] = how many of each
  int classify() {
    for (int k = 0; k < NEXT_NKINDS; k++) cur[k] = 0;
    HIP_TRY(hipMemsetAsync(e->d_count, 0, sizeof(int32_t) * 2 * NEXT_NKINDS, s));
    hipLaunchKernelGGL(k_classify, dim3(nblocks(e->npackets)), dim3(BLOCK), 0, s, env, lists_for(0), std::exchange(first_pass, false) ? 1 : 0);
    return read_counts();
  }
  int64_t count_listed() const { return (int64_t)cnt[NEXT_RPKT] + cnt[NEXT_MA] + cnt[NEXT_SLOW] + cnt[NEXT_KPKT] + cnt[NEXT_GAMMA] + cnt[NEXT_BB]; }
  // chunks of a pull kernel's list (one per wave of its grid, or eight: one per XCD); steps per packet of a launch (the smaller budget for a short list, where one is set)
  static int chunk_count(bool per_wave, int32_t nk, int nwaves) { return per_wave ? chunks_for(nk, nwaves) : 8; }
  int budget_for(int budget, int budget_small, int32_t nk) const { return (budget_small > 0 && nk < e->small_list) ? std::min(budget_small, budget) : budget; }
  // ... and after the launch's list is used up (drain: only where the next launch will be large too, so that what is handed on runs beside a full list)
  int drain_for(int drain, int budget, int32_t nk) const { return (drain > 0 && nk >= e->drain_min_list) ? drain : budget; }
  // DETAILED_BF builds: the estimator updates the launch before recorded (the cells' cache rows are still resident)
  int flush_bf_events() {
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
    if (env.bfev != nullptr) {
      launch_bfest_dense(e, env, s);
      HIP_TRY(hipMemsetAsync(e->d_bfev_count, 0, sizeof(int32_t), s));
    }
#endif
    return ARTIS_OK;
  }
  int launch_rpkt(const int32_t *lst, int32_t nk, const Lists &next) {
    const int grid = (int)std::min<int64_t>(((int64_t)nk + ARTIS_RPKT_TB - 1) / ARTIS_RPKT_TB, (int64_t)e->ncu * ARTIS_RPKT_WGS);  // persistent: every block resident
    const int bud_r = budget_for(e->budget_r, e->budget_r_small, nk);
    const int nch = chunk_count(e->wave_chunks_r, nk, grid * (ARTIS_RPKT_TB / 64));
    const int drain = drain_for(e->drain_r, bud_r, nk);
    const bool rpkt_line_lds = e->line_lds && e->Mh.nlines <= LINE_LDS_MAX && e->Mh.nlines > 0 && !(env.cellest_n_r > RPKT_CELLEST_CAP);
    const bool rpkt_cont_lds = !rpkt_line_lds && e->cont_lds && e->Mh.nbfcontinua <= CONT_LDS_MAX && e->Mh.nbfcontinua > 0 &&
                               !(env.cellest_n_r > RPKT_CELLEST_CAP);
    // (the kernel's own choice, k_rpkt: the workgroup's array for cellest_n_r > 0, else the waves' caches except in the LINE_LDS form)
    e->last.est_forms |= env.cellest_n_r > 0 ? (rpkt_line_lds ? ARTIS_AMD_EST_RPKT_LDS_LINE
                                                              : (rpkt_cont_lds ? ARTIS_AMD_EST_RPKT_LDS_CONT : ARTIS_AMD_EST_RPKT_LDS_NOCONT))
                                             : ((!rpkt_line_lds && env.estcache_on) ? ARTIS_AMD_EST_RPKT_WAVECACHE : ARTIS_AMD_EST_RPKT_GLOBAL);
    auto launch = [&](auto cont_lds, auto line_lds) {
      hipLaunchKernelGGL((k_rpkt<decltype(cont_lds)::value, ARTIS_RPKT_TB, decltype(line_lds)::value>), dim3(grid), dim3(ARTIS_RPKT_TB), 0, s, env, lst, nk,
                         next, e->d_stats, bud_r, e->d_cursors, nch, drain);
    };
    if (rpkt_line_lds)
      launch(std::false_type{}, std::true_type{});
    else if (rpkt_cont_lds)
      launch(std::true_type{}, std::false_type{});
    else
      launch(std::false_type{}, std::false_type{});
    if (ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON && env.bfev == nullptr) e->last.est_forms |= ARTIS_AMD_EST_BF_INPLACE;
    return flush_bf_events();
  }
  int launch_thermal(const int32_t *lst, int32_t nk, const Lists &next) {
    const int bud_t = budget_for(e->budget_t, e->budget_t_small, nk);
    const int drain = drain_for(e->drain_t, bud_t, nk);
    // k_thermal in a launch with the hand-over (drain < bud_t): no unit budget while the list lasts (budget_t_bulk = 0), a packet leaves for budget
    // reasons only once the list is used up, after `drain` units. Launches without hand-over, and k_thermal_q, keep bud_t.
    const int bud_k = (drain < bud_t) ? (e->budget_t_bulk > 0 ? e->budget_t_bulk : INT_MAX) : bud_t;
    const size_t tq_bytes = tq_lds_bytes(TQ_TB, e->Mh.nlevels, e->Mh.nalltrans);
    const bool cold = e->Mh.ncold > 0;  // (kernels built with the on-demand records' look-ups only where the model has cold levels)
    if (cold) e->last.thermal_variants |= ARTIS_AMD_THERMAL_COLD;
    auto launch = [&](auto tb, auto tables_lds, int grid, int nchunks, int chunk_mode) {
      with_flag(cold, [&](auto is_cold) {
        hipLaunchKernelGGL((k_thermal<decltype(tb)::value, decltype(tables_lds)::value, decltype(is_cold)::value>), dim3(grid), dim3(decltype(tb)::value), 0,
                           s, env, lst, nk, next, e->d_stats, bud_k, e->d_cursors, nchunks, chunk_mode, drain);
      });
    };
    const int grid1024 = (int)std::min<int64_t>(((int64_t)nk + 1023) / 1024, (int64_t)e->ncu);
    if (e->thermal_refill && ARTIS_THERMAL_SPLIT_EXACT && env.cellest_n_t == 0 && tq_bytes <= 160 * 1024 - 1024 && nk >= 4096 && e->Mh.nlevels < 32768) {
      e->last.thermal_variants |= ARTIS_AMD_THERMAL_REFILL;
      e->last.est_forms |= ARTIS_AMD_EST_THERMAL_GLOBAL;  // (k_thermal_q keeps no per-cell sums in LDS)
      if (!e->tq_attr_set) {  // (per engine, i.e. per device: the attribute is the device's, not the process's)
        HIP_TRY(hipFuncSetAttribute((const void *)k_thermal_q<TQ_TB, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024));
        HIP_TRY(hipFuncSetAttribute((const void *)k_thermal_q<TQ_TB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024));
        e->tq_attr_set = true;
      }
      const int grid = (int)std::min<int64_t>(((int64_t)nk + TQ_TB - 1) / TQ_TB, (int64_t)e->ncu);
      with_flag(cold, [&](auto is_cold) {
        hipLaunchKernelGGL((k_thermal_q<TQ_TB, decltype(is_cold)::value>), dim3(grid), dim3(TQ_TB), tq_bytes, s, env, lst, nk, next, e->d_stats, bud_t,
                           e->d_cursors, chunk_count(e->wave_chunks_t, nk, grid * (TQ_TB / 64)), drain, e->tq_low);
      });
    } else if (e->ma_tables_lds && e->Mh.nlevels <= MA_LDS_LEVELS && e->Mh.nalltrans <= MA_LDS_TRANS && nk >= 4096) {
      e->last.thermal_variants |= ARTIS_AMD_THERMAL_LDS_TABLES;
      e->last.est_forms |= thermal_est_form(env, 1);
      launch(Int<1024>{}, Int<1>{}, grid1024, chunk_count(e->wave_chunks_t, nk, grid1024 * 16), 0);
    } else if (e->ma_tables_lds && e->Mh.nlevels <= MA_LDS_LEVELS2 && nk >= 4096 && env.cellest_n_t == 0) {
      e->last.thermal_variants |= ARTIS_AMD_THERMAL_LDS_LEVELPACK;
      e->last.est_forms |= thermal_est_form(env, 2);
      launch(Int<1024>{}, Int<2>{}, grid1024, chunk_count(e->wave_chunks_t, nk, grid1024 * 16), 0);
    } else {
      const int grid = (int)std::min<int64_t>(((int64_t)nk + ARTIS_THERMAL_TB - 1) / ARTIS_THERMAL_TB,
                                              (int64_t)e->ncu * std::min(e->thermal_blocks_per_cu, ARTIS_THERMAL_WGS));  // persistent: every workgroup resident
      const bool per_cu = e->cu_chunks_t && nk >= 256 * 1024;
      e->last.thermal_variants |= ARTIS_AMD_THERMAL_PLAIN;
      e->last.est_forms |= thermal_est_form(env, 0);
      launch(Int<ARTIS_THERMAL_TB>{}, Int<0>{}, grid, per_cu ? 256 : chunk_count(e->wave_chunks_t, nk, grid * (ARTIS_THERMAL_TB / 64)), per_cu ? 2 : 0);
    }
    return ARTIS_OK;
  }
  void launch_gamma(const int32_t *lst, int32_t nk, const Lists &next) {
    const int grid = std::min(nblocks(nk), e->ncu * ARTIS_GAMMA_WAVES);
    e->last.est_forms |= env.cellest_n_g > 0 ? ARTIS_AMD_EST_GAMMA_LDS : ARTIS_AMD_EST_GAMMA_GLOBAL;
    hipLaunchKernelGGL(k_gamma, dim3(grid), dim3(BLOCK), 0, s, env, lst, nk, next, e->d_stats, e->budget_g, e->d_cursors,
                       chunk_count(e->wave_chunks_r, nk, grid * (BLOCK / 64)));
  }
  // VPKT builds: the virtual packets of the events the launch of `kind` recorded
  int launch_vpkt_followup([[maybe_unused]] int kind) {
#if ARTIS_OPT_VPKT_ON
    if (kind != NEXT_GAMMA && kind != NEXT_BB) {
      HIP_TRY(hipMemsetAsync(e->d_cursors, 0, sizeof(int32_t) * PULL_SLOTS, s));
      if (e->vpkt_cont_lds && e->Mh.nbfcontinua <= CONT_LDS_MAX && e->Mh.nbfcontinua > 0)
        hipLaunchKernelGGL((k_vpkt<true, ARTIS_VPKT_TB>), dim3(e->ncu), dim3(ARTIS_VPKT_TB), 0, s, env, e->d_stats, e->d_cursors);
      else
        hipLaunchKernelGGL((k_vpkt<false, BLOCK>), dim3(e->ncu * ARTIS_VPKT_WGS), dim3(BLOCK), 0, s, env, e->d_stats, e->d_cursors);
      HIP_TRY(hipMemsetAsync(e->d_vpkt_count, 0, sizeof(int32_t), s));
    }
#endif
    return ARTIS_OK;
  }
  // After a launch (events ev0 .. ev1 around it): the counts, its time, the call's records; the alternate list of `kind` -- what the launch kept of its own
  // kind -- becomes the current one (its count moves on the device: no second sync). tail: k_tail's launch over n packets; `kind` is NEXT_SLOW, the one list it appends to.
  int finish_launch(int kind, bool tail, int32_t n) {
    HIP_TRY(hipEventRecord(e->ev1, s));
    if (!tail) wall_launch += since(t_launch);
    STEP(read_counts());
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->last.nlaunches++;
    (tail ? e->last.kms_tail : e->last.kms[kind]) += ms;
    if (tail) e->last.tail_launches++;
    if (!tail) {
      e->last.klaunches[kind]++;
      e->last.kthreads[kind] += n;
      visit_launches++;
    }
    if (e->trace && tail)
      fprintf(stderr, "[artis_amd] launch %lld tail n=%d+0 %.3f ms -> r %d ma %d slow %d gamma %d bb %d\n", (long long)e->last.nlaunches, n, ms, cnt[NEXT_RPKT], cnt[NEXT_MA], cnt[NEXT_NKINDS], cnt[NEXT_GAMMA], cnt[NEXT_BB]);
    else if (e->trace)
      fprintf(stderr, "[artis_amd] launch %lld kind %d n=%d %.3f ms -> r %d ma %d slow %d k %d self %d\n", (long long)e->last.nlaunches, kind, n, ms, cnt[NEXT_RPKT], cnt[NEXT_MA], cnt[NEXT_SLOW], cnt[NEXT_KPKT], cnt[NEXT_NKINDS]);
    cur[kind] = 1 - cur[kind];
    cnt[kind] = cnt[NEXT_NKINDS];
    HIP_TRY(hipMemcpyAsync(e->d_count + kind, e->d_count + NEXT_NKINDS, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (++guard > 2000000LL) {
      g_last_error = "packet loop did not terminate";
      return ARTIS_ERR_NOTCONVERGED;
    }
    return ARTIS_OK;
  }
  // the last packets of the r-packet, thermal, slow-path and black-body kinds: one launch carries each through all its remaining alternations (k_tail)
  static constexpr int tail_kinds[4] = {NEXT_RPKT, NEXT_MA, NEXT_SLOW, NEXT_BB};
  int64_t count_tail() const { return (int64_t)cnt[NEXT_RPKT] + cnt[NEXT_MA] + cnt[NEXT_SLOW] + cnt[NEXT_BB]; }
  int run_tail(int64_t tail_n) {
    // the four current lists are consumed whole, and no packet comes back to them -- but for one case: a packet that waits for a record of a
    // pool that is used up leaves for the slow-path list (k_tail "waits"). That entry must not land in a buffer other waves still read their
    // packets from: the slow-path kind is the launch's own kind, its entries go to the ALTERNATE slow-path list, which becomes the current one
    // (finish_launch(), as after a launch of the slow-path kernel).
    TailLists in;
    for (int i = 0; i < 4; i++) {
      in.list[i] = e->d_lists[tail_kinds[i]][cur[tail_kinds[i]]];
      in.n[i] = cnt[tail_kinds[i]];
      HIP_TRY(hipMemsetAsync(e->d_count + tail_kinds[i], 0, sizeof(int32_t), s));
    }
    HIP_TRY(hipMemsetAsync(e->d_count + NEXT_NKINDS, 0, sizeof(int32_t), s));
    STEP(reset_pool_if_due());
    HIP_TRY(hipEventRecord(e->ev0, s));
    e->last.thermal_variants |= ARTIS_AMD_THERMAL_TAIL;
    hipLaunchKernelGGL(k_tail, dim3(nblocks(tail_n * 64)), dim3(BLOCK), 0, s, env, in, lists_for(NEXT_SLOW), e->d_stats);
    STEP(flush_bf_events());
    return finish_launch(NEXT_SLOW, true, (int32_t)tail_n);
  }
  // the current list of `kind`, sorted by its keys where lists of that kind are (*lst: the list to launch on; into: sort_by_key())
  int sort_current(int kind, const int32_t **lst, int32_t *into = nullptr) {
    *lst = e->d_lists[kind][cur[kind]];
    if (kind == NEXT_RPKT || kind == NEXT_GAMMA || (kind == NEXT_MA && e->sort_ma)) {
      STEP(sort_by_key(e, s, e->d_lists[kind][cur[kind]], e->d_keys[kind][cur[kind]], cnt[kind], lst,
                       kind == NEXT_RPKT ? r_nubins : (kind == NEXT_MA ? e->ma_bins : 1), e->cc.res.tile_cells,
                       kind == NEXT_MA ? (env.cellest_n_t > 0 ? INT32_MAX : e->sort_maxpc_t) : (env.cellest_n_r > 0 ? INT32_MAX : e->sort_maxpc_r),
                       (kind == NEXT_RPKT && r_nubins > 1 && e->sort_numajor) ? r_ngroups * r_nubins : 0, into));
    }
    return ARTIS_OK;
  }
  bool late_eligible() const { return late_possible(e) && e->d_late_ring[0] != nullptr; }  // (late_possible(): with the packet buffers)
  // The r-packet, the thermal and the slow-path list go to k_late whole (the first two sorted, as for the split kernels: a workgroup's share is
  // local in cell and frequency; the slow-path list as it stands, as for k_slow) and no packet comes back to them: what the kernel ejects goes
  // to the CURRENT blackbody and gamma-ray lists, which no wave reads during the launch (their entries so far stay where they are; the appends
  // follow them).
  int run_late() {
#if ARTIS_LATE_KERNEL
    LateArgs a;
    const int kinds[LATE_NQ] = {NEXT_RPKT, NEXT_MA, NEXT_SLOW};
    const clk::time_point t_sort = clk::now();
    for (int i = 0; i < LATE_NQ; i++) {
      // (the second sort's output must not be the first's: the kind's alternate list is free, this launch has no kind of its own)
      STEP(sort_current(kinds[i], &a.list[i], e->d_lists[kinds[i]][1 - cur[kinds[i]]]));
      a.n[i] = cnt[kinds[i]];
      a.ring[i] = e->d_late_ring[i];
    }
    wall_sort += since(t_sort);
#ifdef ARTIS_PROFILE_LATE
    if (e->d_late_stamp == nullptr) HIP_TRY(hipMalloc((void **)&e->d_late_stamp, sizeof(int32_t) * (size_t)std::max<int64_t>(e->npackets, 1)));
    a.stamp = e->d_late_stamp;
#endif
    a.bailouts = e->d_late_bail;
    a.poll_cap = 1 << 20;  // x s_sleep 64: seconds
    const size_t lds = late_lds_bytes(e->Mh.nlevels, e->Mh.nalltrans, e->Mh.nbfcontinua);
    if (!e->late_attr_set) {  // (per engine, i.e. per device)
      HIP_TRY(hipFuncSetAttribute((const void *)k_late, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024));
      e->late_attr_set = true;
    }
    for (int i = 0; i < LATE_NQ; i++) HIP_TRY(hipMemsetAsync(e->d_count + kinds[i], 0, sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(e->d_late_bail, 0, sizeof(int32_t), s));
    // ABSENT IONS (tables.h): the kernel ejects the packets that wait for a record the population left out to the slow-path list -- the ALTERNATE one
    // (its workgroups still read their shares of the current one), which becomes the current list as after a launch of that kind; run_visit() runs it next
    const bool absent_on = env.ion_absent != nullptr;
    if (absent_on) HIP_TRY(hipMemsetAsync(e->d_count + NEXT_NKINDS, 0, sizeof(int32_t), s));
    HIP_TRY(hipEventRecord(e->ev0, s));
    e->last.thermal_variants |= ARTIS_AMD_THERMAL_LATE;
    hipLaunchKernelGGL(k_late, dim3(e->ncu), dim3(LATE_TB), lds, s, env, a, lists_for(absent_on ? NEXT_SLOW : 0), e->d_stats);
    HIP_TRY(hipEventRecord(e->ev1, s));
    STEP(read_counts());
    if (absent_on) {
      cur[NEXT_SLOW] = 1 - cur[NEXT_SLOW];
      cnt[NEXT_SLOW] = cnt[NEXT_NKINDS];
      HIP_TRY(hipMemcpyAsync(e->d_count + NEXT_SLOW, e->d_count + NEXT_NKINDS, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    }
    const int32_t bail = e->h_counts[(2 * NEXT_NKINDS) + 1];  // (the slot after the error flag: one pinned copy brings all)
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->last.nlaunches++;
    e->last.kms_late += ms;
    e->last.late_launches++;
    e->last.late_bailouts += bail;
    if (e->trace)
      fprintf(stderr, "[artis_amd] launch %lld late n=%d+%d+%d %.3f ms -> slow %d gamma %d bb %d; %d waves gave up waiting\n", (long long)e->last.nlaunches,
              a.n[0], a.n[1], a.n[2], ms, cnt[NEXT_SLOW], cnt[NEXT_GAMMA], cnt[NEXT_BB], bail);
    if (bail != 0 && e->late_strict) {
      g_last_error = "k_late: " + std::to_string(bail) + " waves gave up waiting for work (ARTIS_AMD_LATE_STRICT=1)";
      return ARTIS_ERR_NOTCONVERGED;
    }
    if (++guard > 2000000LL) {
      g_last_error = "packet loop did not terminate";
      return ARTIS_ERR_NOTCONVERGED;
    }
#endif
    return ARTIS_OK;
  }
  // one launch = the whole current list of one kind: sort it, launch its kernel and what follows the kernel
  int run_kind(int kind) {
    const int32_t nk = cnt[kind];
    const Lists next = lists_for(kind);
    const int32_t *lst = e->d_lists[kind][cur[kind]];
    const clk::time_point t_sort = clk::now();
    STEP(sort_current(kind, &lst));
    wall_sort += since(t_sort);
    t_launch = clk::now();
    if (kind == NEXT_SLOW) STEP(reset_pool_if_due());
    // the kernel starts with an empty current list of its own kind: everything it keeps goes to the alternate list
    hipLaunchKernelGGL(k_launch_reset, dim3(1), dim3(BLOCK), 0, s, e->d_count, kind, e->d_cursors);  // (one command instead of three memsets)
    HIP_TRY(hipEventRecord(e->ev0, s));
    if (kind == NEXT_RPKT)
      STEP(launch_rpkt(lst, nk, next));
    else if (kind == NEXT_GAMMA)
      launch_gamma(lst, nk, next);
    else if (kind == NEXT_MA)
      STEP(launch_thermal(lst, nk, next));
    else if (kind == NEXT_BB)
      hipLaunchKernelGGL(k_blackbody, dim3(nblocks(nk)), dim3(BLOCK), 0, s, env, lst, nk, next, e->d_stats);
    else
      hipLaunchKernelGGL(k_slow, dim3(nblocks(nk)), dim3(BLOCK), 0, s, env, lst, nk, next, e->d_stats);
    STEP(launch_vpkt_followup(kind));
    return finish_launch(kind, false, nk);
  }
  // Tiled runs: does the visit leave what is left of it waiting in its cells? (Their state is in the packet store; the next classify pass lists
  // them again.) tail_now: the tail kernel would take them with its next launch.
  bool should_park(int sweep, int tile, int64_t tail_n, bool tail_now) {
    if (!e->park_tails || e->cc.ntiles <= 1 || visit_launches == 0) return false;
    // (round 6) a visit that began larger parks what is left of it once that has fallen to park_at packets -- BEFORE the long run
    // of small, latency-bound launches that its last packets would otherwise cost every visit: they wait in their cells and are listed
    // again, merged with the other windows' stragglers, by a later visit (a visit that BEGINS with that few runs them to their end)
    if (e->park_at > e->tail_max && listed > e->park_at && tail_n > 0 && tail_n + cnt[NEXT_KPKT] <= e->park_at) {
      e->last.parked += tail_n + cnt[NEXT_KPKT] + cnt[NEXT_GAMMA];
      if (e->trace) fprintf(stderr, "[artis_amd] sweep %d tile %d: %lld packets parked (park_at)\n", sweep, tile, (long long)(tail_n + cnt[NEXT_KPKT]));
      return true;
    }
    // a visit that began larger than a tail: its last packets run with the packets that return to the tile in the next sweep, instead of one long
    // k_tail launch per visit. A visit that BEGINS with a tail's worth of packets runs them to their end: no packet waits more than once without
    // the tile's population having shrunk to that.
    if (tail_now && listed > e->tail_max) {
      e->last.parked += tail_n + cnt[NEXT_GAMMA];
      if (e->trace) fprintf(stderr, "[artis_amd] sweep %d tile %d: %lld packets parked\n", sweep, tile, (long long)tail_n);
      return true;
    }
    return false;
  }
  // One visit: launches until every list is empty or the rest is parked. Order: slow path, k-packets, macro-atoms, r-packets, so that a
  // k-packet -> macro-atom -> k-packet cycle costs two launches.
  int run_visit(int sweep, int tile) {
    static constexpr int order[6] = {NEXT_SLOW, NEXT_GAMMA, NEXT_BB, NEXT_KPKT, NEXT_MA, NEXT_RPKT};
    e->last_visits++;
    listed = count_listed();
    e->last.listed += listed;
    visit_launches = 0;
    if (e->trace) fprintf(stderr, "[artis_amd] sweep %d tile %d of %d\n", sweep, tile, e->cc.ntiles);
    // the tail kernel takes the end of a population that began larger (a population that begins below the threshold runs on
    // the split kernels throughout, unless ARTIS_AMD_TAIL_ALWAYS=1)
    // (tiled runs: the later sweeps bring a tile a few stragglers at a time; each such visit is a tail from its first launch)
    const bool tail_ok = e->tail_max > 0 && (e->tail_always || listed > e->tail_max || sweep > 0 || (adaptive && e->last_visits > e->cc.ntiles));
    // k_late takes the r-packets and thermal packets of a population that began larger than late_max once that few are left (same rule; a small
    // population stays on the split kernels unless ARTIS_AMD_LATE_ALWAYS=1), slow-path actions included; the kinds it ejects (blackbody, gamma-ray)
    // run on their own kernels between its launches. An engine that takes k_late has no use for k_tail: k_late ends the population.
    const bool late_ok = late_eligible() && (e->late_always || listed > e->late_max);
    while (count_listed() > 0) {
      // (r-packet + thermal + k-packet lists; and the blackbody list must not be longer than that either: a step's first round has most packets
      // there, about to become r-packets, beside a short thermal list)
      if (late_ok && cnt[NEXT_KPKT] == 0 && (int64_t)cnt[NEXT_RPKT] + cnt[NEXT_MA] <= e->late_max && cnt[NEXT_BB] <= e->late_max) {
        if (cnt[NEXT_RPKT] + cnt[NEXT_MA] + cnt[NEXT_SLOW] > 0) STEP(run_late());
        // (what k_late left on the slow-path list waits for records the population left out: k_slow fills them, tables.h "ABSENT IONS")
        if (env.ion_absent != nullptr && cnt[NEXT_SLOW] > 0) STEP(run_kind(NEXT_SLOW));
        for (int kind : order)
          if (kind == NEXT_GAMMA || kind == NEXT_BB)
            if (cnt[kind] > 0) STEP(run_kind(kind));
        continue;
      }
      const int64_t tail_n = count_tail();
      const bool tail_now = tail_ok && tail_n > 0 && tail_n <= e->tail_max && cnt[NEXT_KPKT] == 0;
      if (should_park(sweep, tile, tail_n, tail_now)) break;
      if (tail_now) {
        STEP(run_tail(tail_n));
        if (env.ion_absent != nullptr && cnt[NEXT_SLOW] > 0) STEP(run_kind(NEXT_SLOW));  // (as after k_late above)
        continue;
      }
      for (int kind : order)
        if (cnt[kind] > 0) STEP(run_kind(kind));
    }
    return ARTIS_OK;
  }
};
}  // namespace
extern "C" int artis_amd_update_packets_device(artis_amd_engine *e, void *hip_stream) {
  if (!e || !e->have_cells || !e->d_pkt) {
    g_last_error = "engine needs artis_amd_set_cellstate() and resident packets first";
    return ARTIS_ERR_ARG;
  }
  HIP_TRY(hipSetDevice(e->device));
  e->fit_since_step = false;
  hipStream_t s = (hipStream_t)hip_stream;
  e->last = {};
  if (e->npackets == 0) return ARTIS_OK;
#ifdef ARTIS_VISIT_COUNTS
  const size_t vb = sizeof(uint32_t) * (size_t)e->Mh.npts_nonempty * (size_t)e->Mh.nlevels;
  if (e->d_visit_counts == nullptr) HIP_TRY(hipMalloc((void **)&e->d_visit_counts, vb));
  HIP_TRY(hipMemsetAsync(e->d_visit_counts, 0, vb, s));
#endif
  if (e->d_absent_counts != nullptr) HIP_TRY(hipMemsetAsync(e->d_absent_counts + 1, 0, sizeof(unsigned long long), s));  // (the records this call fills on demand)
  PropRun run{e, s};
  if (e->d_bfrate_kept != nullptr) {
    if (e->bfrate_kept_dirty)
      HIP_TRY(hipMemsetAsync(e->d_bfrate_kept, 0, sizeof(double) * (size_t)e->Mh.npts_nonempty * (size_t)e->Mh.nbfcontinua, s));
    e->bfrate_kept_dirty = true;
  }
  const PropRun::clk::time_point wall_t0 = PropRun::clk::now();
  if (e->cc.ntiles > 1 && e->cc.d_waiting == nullptr) {
    HIP_TRY(hipMalloc((void **)&e->cc.d_waiting, sizeof(int32_t) * (size_t)(e->Mh.npts_nonempty + 1)));
    e->cc.h_waiting.assign((size_t)e->Mh.npts_nonempty + 1, 0);
  }
  e->last_visits = 0;
  for (int sweep = 0;; sweep++) {
    bool any_active = false, all_done = false;
    for (int tstep = 0; tstep < e->cc.ntiles; tstep++) {
      // sweeps alternate their direction: a packet that left its tile against the direction of one sweep is met by the next
      // one on its way back (with one direction it waits a whole sweep per backward crossing)
      const int tile = (e->tile_zigzag && (sweep & 1)) ? e->cc.ntiles - 1 - tstep : tstep;
      STEP(run.prepare_visit(tile, &all_done));
      if (all_done) break;
      STEP(run.classify());
      if (run.count_listed() == 0) continue;
      any_active = true;
      STEP(run.run_visit(sweep, tile));
    }
    if (any_active) e->last.sweeps++;
    if (e->cc.ntiles == 1 || !any_active || all_done) break;
  }
  for (int k = 1; k < NEXT_NKINDS; k++) e->last.propagate_ms += e->last.kms[k];
  e->last.propagate_ms += e->last.kms_tail + e->last.kms_late;
  if (e->trace)
    fprintf(stderr, "[artis_amd] host time of the call: %.1f ms = %.1f waiting for the stream + %.1f submitting sorts + %.1f submitting launches + the rest; kernels by their events %.1f ms\n",
            PropRun::since(wall_t0), run.wall_sync, run.wall_sort, run.wall_launch, e->last.propagate_ms);
#if ARTIS_OPT_DETAILED_BF_ESTIMATORS_ON
  if (run.env.bfrate_kept != nullptr && run.env.bfev != nullptr)
    hipLaunchKernelGGL(k_bfrate_expand, dim3(nblocks((int64_t)e->Mh.npts_nonempty * 64)), dim3(BLOCK), 0, s, run.env);
  e->bfrate_kept_dirty = false;
#endif
  if (e->Mh.ncold > 0) {  // what the pool of on-demand records holds at the call's end (since its last emptying): artis_amd_last_pool_usage()
    uint32_t used = 0;
    HIP_TRY(hipMemcpy(&used, e->K.ma_pool_used, sizeof(used), hipMemcpyDeviceToHost));
    e->last_pool_used = std::min<int64_t>(used, run.env.ma_pool_cap);
    e->last_pool_cap = run.env.ma_pool_cap;
  }
  if (e->d_absent_counts != nullptr) {  // artis_amd_last_absent_records()
    unsigned long long filled = 0;
    HIP_TRY(hipMemcpy(&filled, e->d_absent_counts + 1, sizeof(filled), hipMemcpyDeviceToHost));
    e->last_absent_filled = (int64_t)filled;
    if (e->trace) fprintf(stderr, "[artis_amd] absent ions: %lld records filled on demand (the last population left %lld out)\n", (long long)filled, (long long)e->last_absent_skipped);
  }
  int32_t err = 0;
  HIP_TRY(hipMemcpy(&err, e->d_err, sizeof(err), hipMemcpyDeviceToHost));
  if (err != 0) {
    g_last_error = errflag_text(err, true);
    return ARTIS_ERR_NOTCONVERGED;
  }
  return ARTIS_OK;
}
#undef STEP
