#!/usr/bin/env python3
"""Cost of the rate-coefficient tables on the device (artis_amd_ratecoeff_compute) on the atomic data of a synthetic model (--preset w7,
w7big or cd23like; classic options; the grid does not enter, so it is kept at 4 cells per axis): the wall time of the call and the
HIP-event time of k_rc_tables, the node totals, the x86 build of the same rules (tests/ratecoeff_host, the stage's own exp / expm1) on
--threads threads, and the host-to-device copy of the ready tables that the stage replaces. Against the arithmetic floor: evaluations x
~110 f64 instructions over the device's f64 vector rate. Run it under a time limit of its own (timeout -k 10 600 python
tools/ratecoeff_timing.py); counters in a run of their own (rocprofv3 --pmc alone). One JSON line.

    python tools/ratecoeff_timing.py [--preset w7] [--repeat 3] [--threads 16] [--items-per-launch 0] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from artis_amd import abi, synth  # noqa: E402

NODE = 61
F64_INSTR_PER_EVAL = 110       # per counted evaluation (61 per integral; alpha_sp and bfcooling share theirs): 19 800 VALU instructions per lane were counted for its 183
F64_LANE_OPS_PER_S = 39.3e12   # MI355X: 78.6 TFLOP/s of f64 vector FMA = 39.3e12 lane instructions per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="w7", choices=("small", "w7", "w7big", "cd23like"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--items-per-launch", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    model, cs, ts, aux = synth.build(args.preset, ncoord=4)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine
    import ratecoeff_common as rc

    eng = engine.Engine(model)
    req = abi.RatecoeffRequest(struct_size=C.sizeof(abi.RatecoeffRequest), install=0, items_per_launch=args.items_per_launch)
    wall, kms = [], []
    for _ in range(args.repeat + 1):  # (the first call allocates the block)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng._check(eng.L.artis_amd_ratecoeff_compute(eng.h, C.byref(req)))
        wall.append((time.perf_counter() - t0) * 1e3)
        stats = abi.RatecoeffStats(struct_size=C.sizeof(abi.RatecoeffStats))
        eng._check(eng.L.artis_amd_ratecoeff_download(eng.h, None, None, None, None, C.byref(stats)))
        kms.append(float(stats.kernel_ms))
    d = eng.ratecoeff_download()
    evals = d["nodes"] * NODE
    floor_ms = evals * F64_INSTR_PER_EVAL / F64_LANE_OPS_PER_S * 1e3
    res = {"preset": args.preset, "levels": int(model["nlevels"]), "continua": d["nbfcontinua"], "covered": d["ncovered"], "tablesize": d["tablesize"],
           "entries": d["nbfcontinua"] * d["tablesize"], "first_call_ms": round(wall[0], 2), "call_ms": [round(x, 3) for x in wall[1:]],
           "k_rc_tables_ms": [round(x, 3) for x in kms[1:]], "integrals": d["integrals"], "nodes": d["nodes"], "at_depth_cap": d["at_depth_cap"],
           "flagged": d["flagged"], "evaluations": evals, "arithmetic_floor_ms": round(floor_ms, 4),
           "kernel_ms_over_floor": round(min(kms[1:]) / max(floor_ms, 1e-9), 2)}
    # the copy the stage replaces: the host's three ready tables to the device (pageable memory, as artis_amd_engine_create takes them)
    tables = [d[k] for k in rc.TABLES if d[k] is not None]
    copy = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        held = [torch.from_numpy(t).to("cuda") for t in tables]
        torch.cuda.synchronize()
        copy.append((time.perf_counter() - t0) * 1e3)
        del held
    res.update(upload_bytes=int(sum(t.nbytes for t in tables)), upload_ms=[round(x, 3) for x in copy])
    eng.close()
    # the x86 build of the same rules
    hm = rc.HostModel(model)
    host = []
    for _ in range(max(1, min(args.repeat, 2))):
        t0 = time.perf_counter()
        h = hm.tables(rc.TBMATH, shared=True, nthreads=args.threads)
        host.append((time.perf_counter() - t0) * 1e3)
    res.update(host_threads=args.threads, host_ms=[round(x, 1) for x in host],
               identical_to_host=bool(all(d[k].tobytes() == h[k].tobytes() for k in rc.TABLES + ("flags",) if d[k] is not None)))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
