// rpkt_round.inc -- the body of one iteration of the r-packet kernels' loop: what a wave does with the packets its lanes hold. ONE text, included by
// k_rpkt and by k_late inside their loops (not a function: the split kernel compiles to exactly the code it had with the body written in place,
// registers and spills included -- profiles/r08/kernel_resources_classic.txt). The including loop provides env, ts_end, have, pi, steps, p, x
// (and tprev under ARTIS_PROFILE) and its policy for where packets go:
//   ROUND_LEAVE(n)          expression: give up a packet that could go on, after n steps in this lane?
//   ROUND_PUT(kind, pi)     statement, reached by the whole wave: a lane that gave up its packet pi (have is false now) hands it on with its
//                           next kind; the other lanes pass NEXT_DONE
    int kind = NEXT_DONE;
    int32_t out_pi = 0;
#ifdef ARTIS_PROFILE
    {  // slot 53: everything outside do_rpkt_step (pull, load, store, append), 54: inside; 55: wave iterations
      const long long now = clock64();
      if ((threadIdx.x & 63) == 0) {
        atomicAdd(&env.stats[53], (stat_t)((now - tprev) >> 4));
        atomicAdd(&env.stats[55], (stat_t)1);
      }
      tprev = now;
    }
#endif
    if (have) {
      bool go = rpkt_can_continue(p, ts_end);
      if (go) {
        go = rpkt_iter<ARTIS_RPKT_SPLIT_ABSORB != 0>(env, p, pi, x);
        steps++;
      }
      if (!go || ROUND_LEAVE(steps)) {
        chi_store(env.P, pi, p, x);
        pkt_store(env.P, pi, p);
        kind = classify(env, p, ts_end);
        out_pi = pi;
        have = false;
      }
    }
#ifdef ARTIS_PROFILE
    {
      const long long now = clock64();
      if ((threadIdx.x & 63) == 0) atomicAdd(&env.stats[54], (stat_t)((now - tprev) >> 4));
      tprev = now;
    }
#endif
    ROUND_PUT(kind, out_pi);
