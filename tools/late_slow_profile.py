#!/usr/bin/env python3
"""How long slow-path packets wait in k_late's third queue, bench workload (ARTIS_AMD_SO = a -DARTIS_PROFILE_LATE build of the options' library;
add -DARTIS_LATE_SLOW_WAVE=0 for the form without a dedicated wave): python tools/late_slow_profile.py [options] [packets]"""
import os, sys, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from artis_amd import abi, synth, engine
options = sys.argv[1] if len(sys.argv) > 1 else "classic"
npk = int(sys.argv[2]) if len(sys.argv) > 2 else 10000000
model, cs, ts, aux = synth.build("w7", ncoord=50, options=options)
pk = synth.make_packets(model, aux, npk, seed_base=1281360349, kpkt_fraction=0.02, seed=99)
est = abi.estimators_for(model, options)
eng = engine.Engine(model, preset=options)
eng.set_cellstate(cs, ts)
eng.update_packets(pk.copy(), est)
s = np.asarray(est.stats).astype(float)
k = eng.last_kernel_ms_by_kind()
eng.close()
print(f"{options}: k_late {k.get('k_late')}, k_slow {k.get('k_slow')}, k_tail {k.get('k_tail')}")
n = max(s[43], 1)
print(f"slow-queue entries served in k_late: {s[43]:.0f}; mean wait {16 * s[42] / n:.0f} clocks; waited longer than 65 536 clocks: {s[44]:.0f} "
      f"({s[44] / n:.3f}), longer than 1 048 576 clocks: {s[45]:.0f} ({s[45] / n:.4f}); passes of the role {s[46]:.0f} "
      f"({s[43] / max(s[46], 1):.2f} packets and {16 * s[47] / max(s[46], 1):.0f} clocks each)")
