#!/usr/bin/env python3
"""Cost of the device radiation-field fit (artis_amd_radfield_fit) at bench scale: the bench model (w7, 50^3 cells, 1e7 packets) of
an options preset with the multibin model (default nltenebular: 256 bins, detailed bound-free estimators) after one resident
timestep, then HIP-event time of the per-cell and the per-bin kernel and the wall time of the call, against the x86 build of the
same rules (tests/radfield_host) on --threads threads over the downloaded estimators and cell state. Also reports the share of
bins whose (T_R, W) is bit-identical to the host's, and the bin counts. One JSON line.

    python tools/radfield_timing.py [--options nltenebular] [--packets 10000000] [--repeat 3] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from artis_amd import abi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--options", default="nltenebular")
    ap.add_argument("--packets", type=int, default=10_000_000)
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    model, cs, ts, aux = synth.build("w7", ncoord=args.ncoord, options=args.options)
    pk = synth.make_packets(model, aux, args.packets, seed_base=1281360349, kpkt_fraction=0.02, seed=99)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine
    import test_radfield_fit_rules as rules

    eng = engine.Engine(model, preset=args.options)
    eng.upload_packets(pk)
    eng.set_cellstate(cs, ts)
    t0 = time.perf_counter()
    eng.step()
    step_ms = (time.perf_counter() - t0) * 1e3
    vol = synth.assocvolume_tmin(model)
    res = {"options": args.options, "cells": model["npts_nonempty"], "packets": args.packets, "step_ms": round(step_ms, 1)}
    wall, cell_ms, bin_ms = [], [], []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        d = eng.radfield_fit(ts.c.mid, ts.c.width, vol)
        wall.append((time.perf_counter() - t0) * 1e3)
        cell_ms.append(d["kernel_ms"][0])
        bin_ms.append(d["kernel_ms"][1])
    res.update(device_call_ms=[round(x, 2) for x in wall], cell_kernel_ms=[round(x, 3) for x in cell_ms],
               bin_kernel_ms=[round(x, 2) for x in bin_ms], totals=d["totals"])
    est = abi.estimators_for(model, args.options)
    eng.download_estimators(est)
    nbf = len(d["bfrate_normed"]) // model["npts_nonempty"] if "bfrate_normed" in d else 0
    nline = len(d["Jb_lu_normed"]) // model["npts_nonempty"] if "Jb_lu_normed" in d else 0
    t0 = time.perf_counter()
    h = rules.host_fit(args.options, model, dict(cs.d), est, ts.c.mid, ts.c.width, vol, nbf=nbf, nline=nline, nthreads=args.threads)
    res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["host_threads"] = args.threads
    if "radfieldbin_T_R" in d:
        Td, Th = d["radfieldbin_T_R"], h["radfieldbin_T_R"]
        same = (Td == Th) & (d["radfieldbin_W"] == h["radfieldbin_W"])
        res["bins"] = int(Td.size)
        res["bins_bit_identical"] = round(float(same.mean()), 6)
        res["bin_T_R_max_rel_diff"] = float(np.max(np.abs(Td - Th) / np.maximum(np.abs(Th), 1.0)))
    res["cell_floats_identical"] = all(np.array_equal(d[k], h[k]) for k in ("TJ", "TR", "Te", "W"))
    res["host_totals"] = h["totals"]
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
