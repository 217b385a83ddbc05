// thermal_round.inc -- the body of one iteration of the thermal kernels' loop (up to ARTIS_MA_PHASE macro-atom transitions, then one k-packet step,
// for every lane that holds a packet). ONE text, included by k_thermal and by k_late inside their loops (see rpkt_round.inc). The including loop
// provides env, ts_end, have, pi, units, p, k, the constant COLD (and tprev, PROF_ADD under ARTIS_PROFILE) and its policy:
//   ROUND_LEAVE(n)          expression: give up a packet that could go on, after n units in this lane?
//   ROUND_BEFORE_LEAVE      statements the whole wave runs between the k-packet phase and that decision
//   ROUND_PUT(kind, pi)     statement, reached by the whole wave: see rpkt_round.inc
    int kind = NEXT_DONE;
    int32_t out_pi = 0;
    // the two phases of thermal_iter() (physics.h), spelled out so that the wave reconverges between them
#ifdef ARTIS_PROFILE
    // wave-cycle accounting (units of 16 clocks) in the spare stats slots 42..47: pull+load | macro-atom phase |
    // k-packet phase | store+append, and the wave-level iteration counts of the two phases
    const long long t0 = clock64();
    PROF_ADD(42, t0 - tprev);
#endif
    bool go = have && thermal_can_continue(p, ts_end);
    if (go) {
      // the loop makes the internal transitions; the process that ends a walk is carried out after it, once per phase
      int j = 0;
      int exit_action = -1;
      const U4 *rec = nullptr;
      if (ma_pending(p) && p.pend == PEND_NONE) ma_prepare<COLD>(env, p, k);  // the record of the current level; the walk carries it on
      while (j < ARTIS_MA_PHASE && exit_action < 0 && ma_pending(p) && p.pend == PEND_NONE) {  // [census: transition loop]
#ifdef ARTIS_PROFILE
        if ((threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) ARTIS_STAT(env, 46);
#endif
        rec = ma_record<COLD>(env, k);
        exit_action = ma_jump_internal<ARTIS_MA_DEFER_EXACT != 0, COLD>(env, p, k, rec);
        j++;
      }
      ma_flush_stats(env, k);
      // (a transition whose search the filters could not decide is finished here, outside the loop: the walk goes on in the
      // next phase)
      if (exit_action == MA_EXIT_FILL) {
        p.pend = PEND_MA_FILL;  // a cold level without a record in this cell: the slow-path kernel fills it (physics.h ma_slow_fill)
      } else if (exit_action == MA_EXIT_DEFER) {
#if ARTIS_THERMAL_SPLIT_EXACT
        // the lines' fine bytes decide all but 1e-6 of these (round 6; tables.h "FINE BYTES"): the walk goes on in the next phase. What they leave:
        if (!ma_jump_deferred_fine<COLD>(env, p, k, rec)) {
          p.pend = PEND_MA_SEARCH;  // the slow-path kernel re-adds the sums and makes the transition (physics.h ma_slow_search)
          p.pend_arg = k.defer;
        }
#else
        ma_jump_deferred(env, p, k, rec);
#endif
      } else if (exit_action >= 0) {
        ma_jump_exit<ARTIS_THERMAL_SPLIT_EXACT != 0>(env, p, pi, k, rec, exit_action);
      }
      if (j > 0) chi_after_ma(p);
      units += j;
    }
#ifdef ARTIS_PROFILE
    const long long t1 = clock64();
    PROF_ADD(43, t1 - t0);
#endif
    if (go) {
      // a pre-k-packet, or a k-packet in a grey cell, leaves for the blackbody kernel (classify() below)
      const bool blackbody = (p.type == ARTIS_TYPE_PRE_KPKT) || k.thick;
      if (kpkt_eligible(p, ts_end) && !blackbody) {
#ifdef ARTIS_PROFILE
        if ((threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) ARTIS_STAT(env, 47);
#endif
        do_kpkt<ARTIS_THERMAL_SPLIT_EXACT != 0>(env, p, pi);
        p.chi_mgi = -1;
        units++;
      }
      go = thermal_can_continue(p, ts_end) && !(blackbody && kpkt_eligible(p, ts_end));
    }
#ifdef ARTIS_PROFILE
    const long long t2 = clock64();
    PROF_ADD(44, t2 - t1);
#endif
    ROUND_BEFORE_LEAVE
    if (have && (!go || ROUND_LEAVE(units))) {
      pkt_store_thermal(env.P, pi, p);  // the hot line; the flight line only if an r-packet was emitted
      kind = classify(env, p, ts_end);
      out_pi = pi;
      have = false;
    }
    ROUND_PUT(kind, out_pi);
    pkt_clear_flight(p);  // a thermal packet never reads them: no live range across iterations
#ifdef ARTIS_PROFILE
    tprev = clock64();
    PROF_ADD(45, tprev - t2);
#endif
