#!/usr/bin/env python3
"""Cost of the first cell state on the device (artis_amd_initial_state, artis_amd_grid_update_initial) at bench scale: the 50^3 bench
grid (w7) and a generated network of kilonova size (synth.decay_network("large"): 3000 nuclides, 21 000 decay paths). Reports the wall
time of artis_amd_initial_state and the HIP-event times of its two kernels, the bytes k_init_cells asks for (an X line per path and
cell, and the cells' inputs and outputs) against the HBM rate, and two yardsticks: the x86 build of the same rules
(tests/initial_state_host) on --threads threads, and the path the two calls replace -- the host computation, artis_amd_set_cellstate of
a seed state and artis_amd_grid_update(use_fit = 0) with host arrays -- against artis_amd_grid_update_initial on an engine without a
cell state.

With --profile DIR it then starts itself three times under rocprofv3, each in a process of its own (--no-host --repeat 1): once with
--kernel-trace --stats for the per-kernel times, once with --pmc FETCH_SIZE and once with --pmc TCC_HIT_sum TCC_MISS_sum for the
counters of k_init_cells, and writes DIR/initial_state_timing.json, DIR/kernel_stats_initial_state.csv and DIR/counters.json. One JSON line.

    python tools/initial_state_timing.py [--ncoord 50] [--network large] [--repeat 2] [--threads 16] [--no-host] [--profile profiles/initial_state]
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
    model = synth.with_meannucmass(model)
    net = synth.decay_network(args.network)
    dm = synth.decay_model(model, cs, aux, net, t_model=synth.DAY)
    em = synth.deposition_model(model, net)
    pm = synth.packet_init_model(model, net, em, tmax=80.0 * synth.DAY, initial_energy=True)
    n, ne, nn, npaths = int(model["npts_nonempty"]), int(model["nelements"]), len(net["nuc_z"]), len(net["path_start"]) - 1
    ts0 = synth.make_timestep(float(model["tmin"]), width_frac=0.05, vmax=float(model["vmax"]), nts=0)
    params = synth.initial_model(model, cs, abi.GREY_FEGROUP_APPROX)
    params.update(tstart=float(ts0.c.mid), nts_first=0, num_grey_timesteps=2, optical_depth_is_thick=1e3, optical_depth_is_thick_vpkt=5e2)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine

    eng = engine.Engine(model)
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    eng.packet_init_setup(pm)
    dec = eng.decay_update(params["tstart"])
    res = {"cells": n, "ngrid": int(model["ngrid"]), "nuclides": nn, "paths": npaths, "rpkt_grey_type": "FEGROUP_APPROX"}
    wall, infos = [], []
    for _ in range(args.repeat + 1):  # the first call is a warm-up (it also allocates the result block)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.initial_state(params)
        wall.append((time.perf_counter() - t0) * 1e3)
        infos.append(eng.initial_state_download(arrays=False))
    res["call_ms"] = [round(x, 3) for x in wall[1:]]
    for k in abi.INITIAL_KERNELS:
        res[f"k_init_{k}_ms"] = [round(i["kernel_ms"][k], 4) for i in infos[1:]]
    res["ncells_branch"] = infos[-1]["ncells_branch"]
    lanes = (n + 63) // 64 * 64
    asked = 4 * lanes * npaths + n * (4 + 4 + 8 + 8 + 4 * ne) + n * (4 * 3 + 8 + 4 * 4)
    best = min(i["kernel_ms"]["cells"] for i in infos[1:])
    res.update(cells_bytes_asked=asked, cells_floor_ms=round(asked / ACHIEVABLE_HBM * 1e3, 4), cells_TBps_asked=round(asked / (best * 1e-3) / 1e12, 3),
               cells_bytes_once=4 * n * nn + n * (4 + 4 + 8 + 8 + 4 * ne) + n * (4 * 3 + 8 + 4 * 4))
    # the hand-over on an engine without a cell state, against the path it replaces with the downloaded arrays
    init = eng.initial_state_download()
    ones = np.ones(n, np.float32)
    t0 = time.perf_counter()
    ga = eng.grid_update_initial(ts0, clumpfactor=ones)
    res["grid_update_initial_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["grid_update_initial_kernel_ms"] = [round(x, 3) for x in ga["kernel_ms"]]
    ni, g = int(model["nions"]), max(int(model["nbfcontinua_ground"]), 1)
    seed = dict(cs.d)
    seed.update(ion_groundlevelpops=np.zeros(n * ni, np.float32), W=ones, thick=np.full(n, abi.CELL_THICK, np.int32), corrphotoionrenorm=np.ones(n * g),
                clumpfactor=ones, ffegrp=np.zeros(n, np.float32))
    b = engine.Engine(model)
    T = init["T_initial"]
    t0 = time.perf_counter()
    b.set_cellstate(abi.CellState(seed), ts0)
    res["replaced_set_cellstate_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    gb = b.grid_update(ts0, dec["rho"], dec["elem_massfracs"].ravel(), init["thick"], use_fit=False, TJ=T, TR=T, W=ones, Te=T, kappagrey=init["kappagrey"],
                       clumpfactor=ones)
    res["replaced_grid_update_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["handover_identical_to_replaced_path"] = bool(all(ga[k].tobytes() == gb[k].tobytes() for k in ("Te", "nne", "ion_groundlevelpops", "ion_partfuncts", "flags")))
    b.close()
    if not args.no_host:
        import initial_common as ic

        host = ic.HostInitial(dm, em, pm, model)
        t0 = time.perf_counter()
        E = host.energy(params["tstart"])["energy_vector"]
        res["host_energy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        Z = np.asarray(model["elem_anumber"], np.int32)
        t0 = time.perf_counter()
        want = host.cells(params, init["energy_vector"], dec["rho"], dec["elem_massfracs"], Z, nthreads=args.threads)
        res["host_cells_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["host_threads"] = args.threads
        res["energy_vector_worst_rel"] = float(np.max(np.abs(init["energy_vector"] - E) / np.where(E > 0, E, 1.0)))
        ulps = np.abs(init["T_initial"].view(np.int32).astype(np.int64) - want["T_initial"].view(np.int32).astype(np.int64))
        res["cells_identical_to_host"] = bool(init["endecay_per_mass"].tobytes() == want["endecay_per_mass"].tobytes() and np.array_equal(init["flags"], want["flags"])
                                              and init["kappagrey"].tobytes() == want["kappagrey"].tobytes() and np.array_equal(init["thick"], want["thick"]))
        res["T_initial_one_ulp_apart"] = int((ulps == 1).sum())
        res["T_initial_worst_ulps"] = int(ulps.max())
    eng.close()
    return res


def profile(args, outdir: str) -> dict:
    """three rocprofv3 runs of this tool, each a fresh process; what could not be read is reported, not hidden"""
    os.makedirs(outdir, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), "--no-host", "--repeat", "1", "--ncoord", str(args.ncoord), "--network", args.network]
    info, counters = {}, {}
    for name, flags in (("trace", ["--kernel-trace", "--stats"]), ("fetch", ["--pmc", "FETCH_SIZE"]), ("tcc", ["--pmc", "TCC_HIT_sum", "TCC_MISS_sum"])):
        tmp = tempfile.mkdtemp(prefix="init_" + name)
        cmd = ["rocprofv3", *flags, "--kernel-include-regex", "k_init_", "--output-format", "csv", "-d", tmp, "--", *child]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        info[name + "_command"] = " ".join([c for c in cmd[:-len(child)] if c not in ("-d", tmp)] + ["python", "tools/initial_state_timing.py"] + child[2:])
        if r.returncode != 0:
            info[name + "_error"] = (r.stderr or r.stdout)[-400:]
            shutil.rmtree(tmp, ignore_errors=True)
            return {"profile": info, "counters": counters}  # (nothing more is started after a failed run)
        if name == "trace":
            found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if found:
                shutil.copy(found[0], os.path.join(outdir, "kernel_stats_initial_state.csv"))
                with open(found[0]) as f:
                    info["kernel_stats"] = {re.search(r"k_init_\w+", row["Name"]).group(0): {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
                                            for row in csv.DictReader(f) if "k_init_" in row["Name"]}
            else:
                info["trace_error"] = "no *kernel_stats.csv written"
        else:
            for path in glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True):
                with open(path) as f:
                    for row in csv.DictReader(f):
                        kern = re.search(r"k_init_\w+", row["Kernel_Name"]).group(0)
                        counters.setdefault(kern, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        shutil.rmtree(tmp, ignore_errors=True)
    c = counters.get("k_init_cells", {})
    if c.get("TCC_HIT_sum") and c.get("TCC_MISS_sum"):
        info["k_init_cells_l2_hit_rate"] = round(c["TCC_HIT_sum"][-1] / (c["TCC_HIT_sum"][-1] + c["TCC_MISS_sum"][-1]), 4)
    if c.get("FETCH_SIZE"):
        info["k_init_cells_fetch_size_kb"] = c["FETCH_SIZE"][-1]
    return {"profile": info, "counters": counters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--network", default="large")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true", help="skip the x86 build (profiler runs)")
    ap.add_argument("--profile", metavar="DIR", help="then the rocprofv3 runs; results under DIR")
    args = ap.parse_args()
    res = measure(args)
    if args.profile:
        prof = profile(args, args.profile)
        res["profile"] = prof["profile"]
        with open(os.path.join(args.profile, "counters.json"), "w") as f:  # per kernel, its dispatches in launch order
            json.dump(prof["counters"], f, indent=1)
        with open(os.path.join(args.profile, "initial_state_timing.json"), "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
