#!/usr/bin/env python3
"""Cost of the device decay and abundance update (artis_amd_decay_update) at bench scale: the 50^3 bench grid (w7) with a generated
network of kilonova size (synth.decay_network("large"): 200 isobaric chains of 15, 3000 nuclides, 21000 decay paths, whose long rows end
on the model's elements). Reports the wall time of the call with and without the nuclides' mass fractions, the HIP-event times of its
three kernels, the set-up's time, the bytes of the three arrays the host path would upload (rho, elem_massfracs, elem_meanweight), and
the x86 build of the same rules (tests/decay_host) on --threads threads over the same data. Per-kernel times and counters: run it with
--no-host under rocprofv3 --kernel-trace --stats, and under rocprofv3 --pmc FETCH_SIZE TCC_HIT_sum TCC_MISS_sum in a run of its own.
One JSON line.

    python tools/decay_update_timing.py [--ncoord 50] [--repeat 3] [--threads 16] [--days 20] [--no-host]
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
from artis_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--days", type=float, default=20.0, help="t_mid - t_model")
    ap.add_argument("--no-host", action="store_true", help="skip the x86 build (profiler runs)")
    args = ap.parse_args()
    model, cs, ts, aux = synth.build("w7", ncoord=args.ncoord)
    net = synth.decay_network("large")
    dm = synth.decay_model(model, cs, aux, net, t_model=synth.DAY)
    n, ne, nn, npaths = int(model["npts_nonempty"]), int(model["nelements"]), len(net["nuc_z"]), len(net["path_start"]) - 1
    in_model = np.isin(net["nuc_z"], model["elem_anumber"])
    ends = net["path_nucindex"][net["path_start"][1:] - 1]
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine

    eng = engine.Engine(model)
    t0 = time.perf_counter()
    eng.decay_setup(dm)
    res = {"cells": n, "elements": ne, "nuclides": nn, "paths": npaths, "nuclides_in_model_elements": int(in_model.sum()),
           "row_entries_in_model_elements": int(in_model[ends].sum()), "setup_ms": round((time.perf_counter() - t0) * 1e3, 1),
           "X_bytes": 4 * n * nn, "host_upload_bytes": 4 * n * (1 + 2 * ne)}
    t_mid = synth.DAY + args.days * synth.DAY
    for key, nuclides in (("update", False), ("update_nuclides", True)):
        wall, kms = [], []
        for _ in range(args.repeat + 1):  # the first call is a warm-up (and, with the nuclides, makes their block)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng._check(eng.L.artis_amd_decay_update(eng.h, t_mid, None, int(nuclides), None))
            wall.append((time.perf_counter() - t0) * 1e3)
            kms.append(eng.decay_download_times())
        res[key + "_call_ms"] = [round(x, 3) for x in wall[1:]]
        for k, name in enumerate(("coeffs", "cells", "nuclides")):
            res[f"{key}_k_decay_{name}_ms"] = [round(x[k], 3) for x in kms[1:]]
    if not args.no_host:
        import decay_common as dc

        host = dc.HostDecay(dm, model)
        t0 = time.perf_counter()
        co = host.coeffs(t_mid)
        res["host_coeffs_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        t0 = time.perf_counter()
        h = host.cells(t_mid, co, nuclides=False, nthreads=args.threads)
        res["host_cells_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["host_threads"] = args.threads
        d = eng.decay_update(t_mid, coeffs=co)
        res["identical_to_host_with_its_coefficients"] = bool(all(d[k].tobytes() == h[k].tobytes() for k in ("rho", "elem_massfracs", "elem_meanweight")))
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
