#!/usr/bin/env python3
"""Cost of the bound-free heating coefficients on the device (artis_amd_bfheating_update) at bench scale: the bench model (w7, 50^3
cells, classic) after one resident timestep and a radiation-field fit; the wall time of the call and the HIP-event time of its two kernels
(k_bfh_ground, k_bfh_levels), the three node totals, the x86 build of the same rules (tests/bfheat_host) on --threads threads over a
sample of the fitted cells, scaled to all of them, and the host-to-device copy of the [cell][level] array the stage replaces. Against the
arithmetic floor: evaluations x ~200 f64 instructions over the device's f64 vector rate. Run it under a time limit of its own
(timeout -k 10 600 python tools/bfheating_timing.py); counters in a run of their own (rocprofv3 --pmc alone). One JSON line.

    python tools/bfheating_timing.py [--packets 1000000] [--ncoord 50] [--repeat 3] [--threads 16] [--host-sample 256] [--out FILE]
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

F64_INSTR_PER_EVAL = 200       # the integrand: table look-up, tb_exp, tb_expm1, eight divisions (an estimate from the source)
F64_LANE_OPS_PER_S = 39.3e12   # MI355X: 78.6 TFLOP/s of f64 vector FMA = 39.3e12 lane instructions per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1_000_000)
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--model", default="w7")
    ap.add_argument("--host-sample", type=int, default=256, help="fitted cells the x86 build computes (its time is scaled to all of them); 0: all")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    model, cs, ts, aux = synth.build(args.model, ncoord=args.ncoord)
    model = synth.with_meannucmass(model)
    state = dict(cs.d)
    pk = synth.make_packets(model, aux, args.packets, seed_base=1281360349, kpkt_fraction=0.02, seed=99)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine
    import bfheat_common as bc

    eng = engine.Engine(model)
    eng.upload_packets(pk)
    eng.set_cellstate(abi.CellState(state), ts)
    eng.step()
    vol = synth.assocvolume_tmin(model)
    n, g, nl = int(model["npts_nonempty"]), int(model["nbfcontinua_ground"]), int(model["nlevels"])
    fit = eng.radfield_fit(ts.c.mid, ts.c.width, vol, lte_iteration=False)
    est = abi.Estimators(n, g)
    eng.download_estimators(est)
    res = {"cells": n, "packets": args.packets, "levels": nl, "phixstargets": int(model["nphixstargets_total"]), "ground_continua": g}
    wall, kms = [], []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p, keep = abi.bfheating_params()
        eng._check(eng.L.artis_amd_bfheating_update(eng.h, C.byref(p), None))
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(eng.bfheating_download(arrays=False)["kernel_ms"])
    d = eng.bfheating_download()
    evals = d["totals"]["nodes"] * bc.NODE
    floor_ms = evals * F64_INSTR_PER_EVAL / F64_LANE_OPS_PER_S * 1e3
    res.update(call_ms=[round(x, 2) for x in wall], ground_ms=[round(k["ground"], 3) for k in kms], levels_ms=[round(k["levels"], 3) for k in kms],
               fitted=d["nfitted"], integrals=d["nintegrals"], totals=d["totals"], evaluations=evals, arithmetic_floor_ms=round(floor_ms, 2),
               levels_ms_over_floor=round(min(k["levels"] for k in kms) / max(floor_ms, 1e-9), 2), cells_flagged=int((d["flags"] != 0).sum()))
    # the copy the stage replaces: the host's [cell][level] doubles to the device (pageable memory, as artis_amd_thermal_solve takes them)
    copy = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = torch.from_numpy(d["coeffs"]).to("cuda")
        torch.cuda.synchronize()
        copy.append((time.perf_counter() - t0) * 1e3)
        del t
    res.update(upload_bytes=int(d["coeffs"].nbytes), upload_ms=[round(x, 2) for x in copy])
    # the x86 build of the same rules, on a sample of the fitted cells (evenly spread; the others are handed over as unfitted)
    fitted = (fit["flags"] & abi.RADFIELD_FITTED) != 0
    sample = np.nonzero(fitted)[0]
    if args.host_sample and len(sample) > args.host_sample:
        sample = sample[np.linspace(0, len(sample) - 1, args.host_sample).astype(np.int64)]
    flags_h = np.zeros(n, np.int32)
    flags_h[sample] = abi.RADFIELD_FITTED
    hm = bc.HostModel(model)
    raw = np.asarray(est.bfheatingestimator).reshape(n, g).copy()
    ins = bc.call_inputs(model, state, ts, dict(fit, flags=flags_h), raw, vol)
    t0 = time.perf_counter()
    h = hm.update(ins, nthreads=args.threads)
    host_ms = (time.perf_counter() - t0) * 1e3
    scaled = host_ms * int(d["nfitted"]) / max(len(sample), 1)
    res.update(host_threads=args.threads, host_sample=int(len(sample)), host_sample_ms=round(host_ms, 1), host_ms_scaled=round(scaled, 1),
               host_path_ms=round(scaled + min(copy), 1),
               identical_to_host=bool(d["coeffs"][sample].tobytes() == h["coeffs"][sample].tobytes() and d["renorm"][sample].tobytes() == h["renorm"][sample].tobytes()))
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
