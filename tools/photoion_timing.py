#!/usr/bin/env python3
"""Cost of the photoionisation coefficients on the device (artis_amd_set_cellstate_photoion) at bench scale: the bench model (w7, 50^3
cells) with the options of nltenebular and synth.nebular_cellstate, estimators off (every entry is an integral): the wall time of the
call (upload of the state, k_photoion, cell-cache population), the HIP-event time of k_photoion, the totals, the x86 build of the same
rules (tests/photoion_host) on --threads threads over a sample of the cells, scaled to all of them, and the host-to-device copy of the
ready [cell][nphixstargets_total] array the call replaces. Against the arithmetic floor: evaluations x ~300 f64 instructions over the
device's f64 vector rate. Run it under a time limit of its own (timeout -k 10 900 python tools/photoion_timing.py). One JSON line.

    python tools/photoion_timing.py [--ncoord 50] [--model w7] [--repeat 3] [--threads 16] [--host-sample 512] [--out FILE]
    python tools/photoion_timing.py --profile DIR [...]   # no timing of its own: a rocprofv3 --kernel-trace --stats run of this tool, then
                                                          # a separate --pmc run (counters are never collected together with tracing)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from artis_amd import abi, synth  # noqa: E402

NODE = 61
F64_INSTR_PER_EVAL = 300       # the integrand: table look-up, tb_exp, tb_expm1, bin selection, seven divisions (an estimate from the source)
F64_LANE_OPS_PER_S = 39.3e12   # MI355X: 78.6 TFLOP/s of f64 vector FMA = 39.3e12 lane instructions per second
PRESET = "nltenebular"
NTS = 13
PMC = ["SQ_WAVES", "SQ_BUSY_CYCLES", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_LDS", "SQ_WAIT_INST_ANY", "GRBM_GUI_ACTIVE"]


def profile(args) -> None:
    """two child processes of this tool under rocprofv3: the kernel trace with statistics, then the counters alone"""
    os.makedirs(args.profile, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--ncoord", str(args.ncoord), "--model", args.model, "--repeat", "1", "--host-sample", "-1"]
    for name, flags in (("trace", ["--kernel-trace", "--stats"]), ("pmc", ["--pmc", *PMC])):
        subprocess.run(["rocprofv3", *flags, "-d", os.path.join(args.profile, name), "--output-format", "csv", "--", *me], check=True, timeout=900)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--model", default="w7")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-sample", type=int, default=512, help="cells the x86 build computes (its time is scaled to all of them); 0: all; -1: none")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--profile", default=None, metavar="DIR", help="run this tool under rocprofv3 into DIR instead (trace and counters in separate runs)")
    args = ap.parse_args()
    if args.profile:
        return profile(args)
    model, cs, ts, aux = synth.build(args.model, ncoord=args.ncoord, options=PRESET, nts=NTS)
    cells = {k: v for k, v in cs.d.items() if k != "corrphotoioncoeff"}
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine

    eng = engine.Engine(model, preset=PRESET)
    state = abi.CellState(cells)
    wall, kms = [], []
    for _ in range(args.repeat + 1):  # (the first call allocates the block)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.set_cellstate_photoion(state, ts, use_bf_estimators=False)
        wall.append((time.perf_counter() - t0) * 1e3)
        info = abi.PhotoionResult(struct_size=abi.C.sizeof(abi.PhotoionResult))
        eng._check(eng.L.artis_amd_photoion_download(eng.h, abi.C.byref(info)))
        kms.append(float(info.kernel_ms))
    d = eng.photoion()
    t = d["totals"]
    evals = t["nodes"] * NODE
    floor_ms = evals * F64_INSTR_PER_EVAL / F64_LANE_OPS_PER_S * 1e3
    n, ne = d["npts_nonempty"], d["nphixstargets_total"]
    res = {"preset": PRESET, "model": args.model, "cells": n, "levels": int(model["nlevels"]), "continua": d["nbfcontinua"], "phixstargets": ne,
           "first_call_ms": round(wall[0], 1), "call_ms": [round(x, 1) for x in wall[1:]], "k_photoion_ms": [round(x, 2) for x in kms[1:]],
           "totals": t, "evaluations": evals, "arithmetic_floor_ms": round(floor_ms, 2),
           "kernel_ms_over_floor": round(min(kms[1:]) / max(floor_ms, 1e-9), 2)}
    # what the call replaces on the device's side: set_cellstate with the ready array (its upload is part of that call), and the array's copy alone
    ready = abi.CellState({**cells, "corrphotoioncoeff": d["coeff"].ravel()})
    given, copy = [], []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.set_cellstate(ready, ts)
        given.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        held = torch.from_numpy(d["coeff"]).to("cuda")
        torch.cuda.synchronize()
        copy.append((time.perf_counter() - t0) * 1e3)
        del held
    res.update(set_cellstate_with_array_ms=[round(x, 1) for x in given], upload_bytes=int(d["coeff"].nbytes), upload_ms=[round(x, 1) for x in copy])
    eng.close()
    if args.host_sample >= 0:
        # the x86 build of the same rules over the first cells (the harness takes its number of cells from the model)
        import photoion_common as pc

        s = n if args.host_sample == 0 else min(args.host_sample, n)
        per_cell = {k: len(np.asarray(v).ravel()) // n for k, v in cells.items() if k in pc.INPUTS}
        sample = {k: np.asarray(cells[k]).ravel()[: s * per_cell[k]] for k in per_cell}
        hm = pc.HostModel(abi.Model({**model.d, "npts_nonempty": s}), PRESET)
        host = []
        for _ in range(max(1, min(args.repeat, 2))):
            t0 = time.perf_counter()
            h = hm.compute(pc.call_inputs(sample, nts=NTS), nthreads=args.threads)
            host.append((time.perf_counter() - t0) * 1e3)
        res.update(host_threads=args.threads, host_cells=s, host_ms_sample=[round(x, 1) for x in host],
                   host_ms_scaled=round(min(host) * n / s, 1), identical_to_host=bool(d["coeff"][:s].tobytes() == h["coeff"].tobytes()))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
