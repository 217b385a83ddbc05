#!/usr/bin/env python3
"""Cost of the device deposition update (artis_amd_deposition_update) at bench scale: the 50^3 bench grid (w7) with a generated network
of kilonova size (synth.decay_network("large"): 3000 nuclides, 2800 of them radioactive). Reports the wall time of the call, the
HIP-event times of its three kernels, the set-up's time, the bandwidth floor of k_dep_cells (the bytes of the radioactive nuclides' X
lines / 6.3 TB/s), and the x86 build of the same rules (tests/deposition_host) on --threads threads over the same data.

With --profile DIR it then starts itself three times under rocprofv3, each in a process of its own (--no-host --repeat 1): once with
--kernel-trace --stats for the per-kernel times, once with --pmc FETCH_SIZE and once with --pmc TCC_HIT_sum TCC_MISS_sum for the
counters of the k_dep_* kernels, and writes DIR/deposition_timing.json, DIR/kernel_stats_deposition.csv and DIR/counters.json.
One JSON line.

    python tools/deposition_timing.py [--ncoord 50] [--repeat 3] [--threads 16] [--days 20] [--no-host] [--profile profiles/deposition]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from artis_amd import abi, synth  # noqa: E402

ACHIEVABLE_HBM = 6.3e12  # B/s


def measure(args) -> dict:
    model, cs, ts, aux = synth.build("w7", ncoord=args.ncoord)
    net = synth.decay_network("large")
    dm = synth.decay_model(model, cs, aux, net, t_model=synth.DAY)
    em = synth.deposition_model(model, net)
    n, nn = int(model["npts_nonempty"]), len(net["nuc_z"])
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine

    eng = engine.Engine(model)
    eng.set_cellstate(cs, ts)
    eng.decay_setup(dm)
    t0 = time.perf_counter()
    eng.deposition_setup(em)
    res = {"cells": n, "nuclides": nn, "setup_ms": round((time.perf_counter() - t0) * 1e3, 1)}
    t_mid = synth.DAY + args.days * synth.DAY
    d = eng.decay_update(t_mid)
    nts = int(ts.c.nts)
    p, keep = abi.deposition_params(ts.c.mid, ts.c.width, nts, nts + 1, nts + 2, 1.0)
    wall, kms = [], []
    for _ in range(args.repeat + 1):  # the first call is a warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng._check(eng.L.artis_amd_deposition_update(eng.h, p, None))
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(eng.deposition_download(arrays=False)["kernel_ms"])
    out = eng.deposition_download()
    nrad = out["nradioactive"]
    x_bytes = 4 * ((n + 63) // 64 * 64) * nrad
    res.update(radioactive=nrad, X_line_bytes=x_bytes, bandwidth_floor_ms=round(x_bytes / ACHIEVABLE_HBM * 1e3, 4),
               update_call_ms=[round(x, 3) for x in wall[1:]])
    for k, name in enumerate(("powers", "cells", "totals")):
        res[f"k_dep_{name}_ms"] = [round(x[k], 3) for x in kms[1:]]
    res["k_dep_cells_TBps"] = round(x_bytes / (min(x[1] for x in kms[1:]) * 1e-3) / 1e12, 3)
    if not args.no_host:
        import deposition_common as dp

        host = dp.HostDep(dm, em, model)
        raw = np.zeros((4, n))
        step = dp.step_params(model, t_mid, ts.c.mid, ts.c.width, nts + 1, nts + 2, 1.0)
        kappagrey = np.asarray(cs["kappagrey"], np.float32)
        t0 = time.perf_counter()
        P = host.vectors(d)
        res["host_vectors_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        t0 = time.perf_counter()
        h = host.cells(step, P, d["rho"], kappagrey, raw, nthreads=args.threads)
        res["host_cells_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        tot, mtot = host.totmass()
        res["host_totmass_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        totals = host.totals(1, P, raw, tot)
        res["host_totals_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res["host_threads"] = args.threads
        same = all(np.asarray(out[k]).tobytes() == np.asarray(h[k]).tobytes() for k in h) and out["power_vectors"].tobytes() == P.tobytes()
        same = same and out["totmassnuclide"].tobytes() == tot.tobytes() and np.array([out["totals"][k] for k in abi.DEP_TOTALS]).tobytes() == totals.tobytes()
        res["identical_to_host"] = bool(same)
    eng.close()
    return res


def profile(args, outdir: str) -> dict:
    """three rocprofv3 runs of this tool, each a fresh process; what could not be read is reported, not hidden"""
    os.makedirs(outdir, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), "--no-host", "--repeat", "1", "--ncoord", str(args.ncoord), "--days", str(args.days)]
    info = {}
    counters = {}
    for name, flags in (("trace", ["--kernel-trace", "--stats"]), ("fetch", ["--pmc", "FETCH_SIZE"]), ("tcc", ["--pmc", "TCC_HIT_sum", "TCC_MISS_sum"])):
        tmp = tempfile.mkdtemp(prefix="dep_" + name)
        cmd = ["rocprofv3", *flags, "--kernel-include-regex", "k_dep_", "--output-format", "csv", "-d", tmp, "--", *child]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        info[name + "_command"] = " ".join(cmd[:-len(child)] + ["python", "tools/deposition_timing.py"] + child[2:])
        if r.returncode != 0:
            info[name + "_error"] = (r.stderr or r.stdout)[-400:]
            shutil.rmtree(tmp, ignore_errors=True)
            return {"profile": info, "counters": counters}  # (nothing more is started after a failed run)
        if name == "trace":
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if found:
                shutil.copy(found[0], os.path.join(outdir, "kernel_stats_deposition.csv"))
                with open(found[0]) as f:
                    info["kernel_stats"] = {re.search(r"k_dep_\w+", row["Name"]).group(0): {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
                                            for row in csv.DictReader(f) if "k_dep_" in row["Name"]}
            else:
                info["trace_error"] = "no *kernel_stats.csv written"
        else:
            for path in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
                with open(path) as f:
                    for row in csv.DictReader(f):
                        kern = re.search(r"k_dep_\w+", row["Kernel_Name"]).group(0)
                        counters.setdefault(kern, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        shutil.rmtree(tmp, ignore_errors=True)
    c = counters.get("k_dep_cells", {})
    if c.get("TCC_HIT_sum") and c.get("TCC_MISS_sum"):
        hit, miss = c["TCC_HIT_sum"][-1], c["TCC_MISS_sum"][-1]
        info["k_dep_cells_l2_hit_rate"] = round(hit / (hit + miss), 4)
    if c.get("FETCH_SIZE"):
        info["k_dep_cells_fetch_size_kb"] = c["FETCH_SIZE"][-1]
    return {"profile": info, "counters": counters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--days", type=float, default=20.0, help="t_mid - t_model")
    ap.add_argument("--no-host", action="store_true", help="skip the x86 build (profiler runs)")
    ap.add_argument("--profile", metavar="DIR", help="then the rocprofv3 runs; results under DIR")
    args = ap.parse_args()
    res = measure(args)
    if args.profile:
        prof = profile(args, args.profile)
        res["profile"] = prof["profile"]
        with open(os.path.join(args.profile, "counters.json"), "w") as f:  # per kernel, its dispatches in launch order
            json.dump(prof["counters"], f, indent=1)
        with open(os.path.join(args.profile, "deposition_timing.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
