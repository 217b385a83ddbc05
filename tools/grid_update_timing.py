#!/usr/bin/env python3
"""Cost of the device ion balance and hand-over (artis_amd_grid_update) at bench scale: the bench model (w7, 50^3 cells, 1e7 packets)
of an options preset without NLTE populations (classic or kilonova_lte) after one resident timestep and a radiation-field fit, then
the HIP-event time of its kernel groups (gamma + partition functions, phi, per-cell solve) and of the cell-cache fill, and the wall
time of the call; against the time of artis_amd_set_cellstate with the same arrays (upload plus fill: what the call replaces) and the
x86 build of the same rules (tests/ionbal_host) on --threads threads over the downloaded inputs. Per-kernel times: run it under
rocprofv3 --kernel-trace --stats. One JSON line.

    python tools/grid_update_timing.py [--options classic] [--packets 10000000] [--repeat 3] [--threads 16]
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
    ap.add_argument("--options", default="classic", choices=("classic", "kilonova_lte"))
    ap.add_argument("--packets", type=int, default=10_000_000)
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--lte", action="store_true", help="the fit and the balance as an LTE iteration (forced Saha in every cell)")
    args = ap.parse_args()
    model, cs, ts, aux = synth.build("w7", ncoord=args.ncoord, options=args.options)
    if args.options == "classic":
        model = synth.with_meannucmass(model)
    state = dict(cs.d)
    if args.options == "kilonova_lte":
        state["elem_meanweight"] = synth.next_matter(model, cs, aux["t"], aux["t"], args.options)["elem_meanweight"]
    pk = synth.make_packets(model, aux, args.packets, seed_base=1281360349, kpkt_fraction=0.02, seed=99)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine
    import ionbal_common as ib

    eng = engine.Engine(model, preset=args.options)
    eng.upload_packets(pk)
    eng.set_cellstate(abi.CellState(state), ts)
    t0 = time.perf_counter()
    eng.step()
    step_ms = (time.perf_counter() - t0) * 1e3
    vol = synth.assocvolume_tmin(model)
    n, g = int(model["npts_nonempty"]), int(model["nbfcontinua_ground"])
    ts_next = synth.make_timestep(ts.c.start + ts.c.width, width_frac=0.05, vmax=model["vmax"], nts=ts.c.nts + 1)
    nm = synth.next_matter(model, abi.CellState(state), ts.c.mid, ts_next.c.mid, args.options)
    d_fit = eng.radfield_fit(ts.c.mid, ts.c.width, vol, lte_iteration=args.lte)
    est = abi.Estimators(n, g)
    eng.download_estimators(est)
    res = {"options": args.options, "cells": n, "packets": args.packets, "lte": args.lte, "step_ms": round(step_ms, 1)}
    wall, kms = [], []
    for _ in range(args.repeat):
        eng.set_cellstate(abi.CellState(state), ts)  # the same input state for every call (the fit's results stay)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = eng.grid_update(ts_next, nm["rho"], nm["elem_massfracs"], nm["thick"], elem_meanweight=nm["elem_meanweight"])
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(d["kernel_ms"])
    res.update(call_ms=[round(x, 2) for x in wall], partfunct_gamma_ms=[round(k[0], 3) for k in kms], phi_ms=[round(k[1], 3) for k in kms],
               solve_ms=[round(k[2], 3) for k in kms], cache_fill_ms=[round(k[3], 2) for k in kms], flags=d["ncells_flagged"],
               evals_per_cell=round(d["total_evals"] / n, 2))
    # what the call replaces: the same arrays through artis_amd_set_cellstate (upload + cell-cache fill)
    s = dict(state)
    for k in ("Te", "TJ", "TR", "W", "nne", "nnetot", "rho"):
        s[k] = d[k]
    s.update(ion_partfuncts=d["ion_partfuncts"].ravel(), ion_groundlevelpops=d["ion_groundlevelpops"].ravel(), elem_massfracs=nm["elem_massfracs"])
    cs_next = abi.CellState(s)
    setc = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.set_cellstate(cs_next, ts_next)
        setc.append((time.perf_counter() - t0) * 1e3)
    res["set_cellstate_ms"] = [round(x, 2) for x in setc]
    # the x86 build of the rules on the same inputs
    hm = ib.HostModel(model, args.options)
    gamma = ib.gamma_normed(np.asarray(est.gammaestimator).reshape(n, g), vol, ts.c.mid, float(model["tmin"]), ts.c.width)
    forced = (np.full(n, args.lte) | (np.asarray(state["thick"]) == ib.CELL_THICK)).astype(np.int32)
    t0 = time.perf_counter()
    h = hm.balance(d_fit["TJ"], d_fit["Te"], forced, state["ion_groundlevelpops"], nm["elem_massfracs"], nm["elem_meanweight"], nm["rho"],
                   state["clumpfactor"], gamma, nthreads=args.threads)
    res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["host_threads"] = args.threads
    same_U = (d["ion_partfuncts"] == h["U"]).all(axis=1)
    res["cells_identical_to_host"] = round(float((same_U & (d["nne"] == h["nne"]) & (d["ion_groundlevelpops"] == h["ground"]).all(axis=1)).mean()), 6)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
