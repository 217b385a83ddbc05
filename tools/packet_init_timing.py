#!/usr/bin/env python3
"""Cost of the device pellet initialisation (artis_amd_packet_init) at bench scale: the 50^3 bench grid (w7), 1e7 packets, a generated
network of kilonova size (synth.decay_network("large"): 3000 nuclides, 21 000 decay paths). Reports the wall time of the call and the
HIP-event times of its kernels against two yardsticks -- the x86 build of the same rules (tests/packet_init_host) on --threads threads,
and the artis_amd_packets_upload of the same population, which the call replaces -- and the checkpoint kernel's bytes (the X lines of
every path's top nuclide and the checkpoints it writes) against its bandwidth floor at 6.3 TB/s.

With --profile DIR it then starts itself three times under rocprofv3, each in a process of its own (--no-host --repeat 1): once with
--kernel-trace --stats for the per-kernel times, once with --pmc FETCH_SIZE and once with --pmc TCC_HIT_sum TCC_MISS_sum for the
counters of the k_pinit_* kernels, and writes DIR/packet_init_timing.json, DIR/kernel_stats_packet_init.csv and DIR/counters.json.
One JSON line.

    python tools/packet_init_timing.py [--ncoord 50] [--npackets 10000000] [--network large] [--repeat 2] [--threads 16] [--trials 0] [--no-host] [--profile profiles/packet_init]
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
SEED_BASE = 12345


def measure(args) -> dict:
    model, cs, ts, aux = synth.build("w7", ncoord=args.ncoord)
    net = synth.decay_network(args.network)
    dm = synth.decay_model(model, cs, aux, net, t_model=synth.DAY)
    em = synth.deposition_model(model, net)
    pm = synth.packet_init_model(model, net, em, tmax=80.0 * synth.DAY, initial_energy=True, max_trials_per_launch=args.trials)
    n, nn, npaths = int(model["npts_nonempty"]), len(net["nuc_z"]), len(net["path_start"]) - 1
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine

    eng = engine.Engine(model)
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    t0 = time.perf_counter()
    eng.packet_init_setup(pm)
    res = {"cells": n, "ngrid": int(model["ngrid"]), "nuclides": nn, "paths": npaths, "npackets": args.npackets, "max_trials_per_launch": args.trials or 4096, "setup_ms": round((time.perf_counter() - t0) * 1e3, 1)}
    wall, infos = [], []
    for _ in range(args.repeat + 1):  # the first call is a warm-up (it also allocates the packet records)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = eng.packet_init(args.npackets, SEED_BASE)
        wall.append((time.perf_counter() - t0) * 1e3)
        infos.append(info)
    res["call_ms"] = [round(x, 2) for x in wall[1:]]
    for k in abi.PINIT_KERNELS:
        res[f"{k}_ms"] = [round(i["kernel_ms"][k], 3) for i in infos[1:]]
    res.update(continuation_launches=infos[-1]["continuation_launches"], max_trials=infos[-1]["max_trials"], e_ratio=infos[-1]["e_ratio"],
               ncheckpoints=infos[-1]["ncheckpoints"])
    nck = infos[-1]["ncheckpoints"]
    lanes = (n + 63) // 64 * 64
    ck_bytes = 4 * lanes * npaths + 8 * n * (nck + 1)
    best = min(i["kernel_ms"]["checkpoints"] for i in infos[1:])
    res.update(checkpoint_bytes=ck_bytes, checkpoint_floor_ms=round(ck_bytes / ACHIEVABLE_HBM * 1e3, 4), checkpoint_TBps=round(ck_bytes / (best * 1e-3) / 1e12, 3))
    # the call this one replaces: the same population from the host
    pk = np.zeros(args.npackets, abi.PACKET_DTYPE)
    eng.download_packets(pk)
    up = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.upload_packets(pk)
        up.append((time.perf_counter() - t0) * 1e3)
    res["upload_ms"] = [round(x, 2) for x in up]
    res["upload_bytes"] = int(pk.nbytes)
    if not args.no_host:
        import packet_init_common as pc

        dl = eng.packet_init_download(per_packet=True)
        host = pc.HostPinit(dm, em, pm, model)
        t0 = time.perf_counter()
        E = host.energy()
        res["host_energy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        cells = host.cells(dl["energy_vector"], nthreads=args.threads)
        res["host_cells_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        t0 = time.perf_counter()
        ref = host.run(args.npackets, seed_base=SEED_BASE, nthreads=args.threads)
        res["host_packets_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["host_threads"] = args.threads
        res["energy_vector_worst_rel"] = float(np.max(np.abs(dl["energy_vector"] - E) / np.where(E > 0, E, 1.0)))
        same = dl["en_cumulative"].tobytes() == cells["en_cumulative"].tobytes()
        for f in ("cellindex", "rngstate", "pellet_nucindex", "pellet_decaytype", "originated_from_particlenotgamma", "nu_cmf", "pos"):
            same = same and bool(np.array_equal(pk[f], ref["packets"][f]))
        res["discrete_identical_to_host"] = bool(same and np.array_equal(dl["channel"], ref["channel"]) and np.array_equal(dl["trials"], ref["trials"]))
    eng.close()
    return res


def profile(args, outdir: str) -> dict:
    """three rocprofv3 runs of this tool, each a fresh process; what could not be read is reported, not hidden"""
    os.makedirs(outdir, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), "--no-host", "--repeat", "1", "--ncoord", str(args.ncoord), "--npackets", str(args.npackets), "--network", args.network, "--trials", str(args.trials)]
    info = {}
    counters = {}
    for name, flags in (("trace", ["--kernel-trace", "--stats"]), ("fetch", ["--pmc", "FETCH_SIZE"]), ("tcc", ["--pmc", "TCC_HIT_sum", "TCC_MISS_sum"])):
        tmp = tempfile.mkdtemp(prefix="pinit_" + name)
        cmd = ["rocprofv3", *flags, "--kernel-include-regex", "k_pinit_", "--output-format", "csv", "-d", tmp, "--", *child]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        info[name + "_command"] = " ".join([c for c in cmd[:-len(child)] if c not in ("-d", tmp)] + ["python", "tools/packet_init_timing.py"] + child[2:])
        if r.returncode != 0:
            info[name + "_error"] = (r.stderr or r.stdout)[-400:]
            shutil.rmtree(tmp, ignore_errors=True)
            return {"profile": info, "counters": counters}  # (nothing more is started after a failed run)
        if name == "trace":
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if found:
                shutil.copy(found[0], os.path.join(outdir, "kernel_stats_packet_init.csv"))
                with open(found[0]) as f:
                    info["kernel_stats"] = {re.search(r"k_pinit_\w+", row["Name"]).group(0): {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
                                            for row in csv.DictReader(f) if "k_pinit_" in row["Name"]}
            else:
                info["trace_error"] = "no *kernel_stats.csv written"
        else:
            for path in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
                with open(path) as f:
                    for row in csv.DictReader(f):
                        kern = re.search(r"k_pinit_\w+", row["Kernel_Name"]).group(0)
                        counters.setdefault(kern, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        shutil.rmtree(tmp, ignore_errors=True)
    for kern in ("k_pinit_checkpoints", "k_pinit_decay"):
        c = counters.get(kern, {})
        if c.get("TCC_HIT_sum") and c.get("TCC_MISS_sum"):  # (of the largest dispatch: k_pinit_decay's continuation launches are tiny)
            hit, miss = max(zip(c["TCC_HIT_sum"], c["TCC_MISS_sum"]), key=sum)
            info[kern + "_l2_hit_rate"] = round(hit / (hit + miss), 4)
        if c.get("FETCH_SIZE"):
            info[kern + "_fetch_size_kb"] = max(c["FETCH_SIZE"])
    return {"profile": info, "counters": counters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--npackets", type=int, default=10000000)
    ap.add_argument("--network", default="large")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--trials", type=int, default=0, help="max_trials_per_launch of the set-up (0: the library's default, 4096)")
    ap.add_argument("--no-host", action="store_true", help="skip the x86 build (profiler runs)")
    ap.add_argument("--profile", metavar="DIR", help="then the rocprofv3 runs; results under DIR")
    args = ap.parse_args()
    res = measure(args)
    if args.profile:
        prof = profile(args, args.profile)
        res["profile"] = prof["profile"]
        with open(os.path.join(args.profile, "counters.json"), "w") as f:  # per kernel, its dispatches in launch order
            json.dump(prof["counters"], f, indent=1)
        with open(os.path.join(args.profile, "packet_init_timing.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
