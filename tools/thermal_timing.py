#!/usr/bin/env python3
"""Cost of the device thermal balance of the thin cells (artis_amd_thermal_solve) at bench scale: the bench model (w7, 50^3 cells, 1e7
packets, classic) after one resident timestep and a radiation-field fit, with the synthetic heating inputs of the tests
(tests/thermal_common.py heating_inputs); the wall time of the call and the HIP-event time of its kernel groups (renormalisation,
Gamma + partition functions, the wave-per-cell solve), the residual evaluations per fitted cell, the share of lane slots that idle in
the strided lists (the downward entries of alltrans and the ends of every list), and the x86 build of the same rules
(tests/thermal_host) on --threads threads over the downloaded inputs. Per-kernel times: run it under rocprofv3 --kernel-trace --stats
(counters in a run of their own). One JSON line.

    python tools/thermal_timing.py [--packets 10000000] [--ncoord 50] [--repeat 3] [--threads 16]
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


def idle_lane_share(model) -> float:
    """of the lane slots of one evaluation's strided sums (64 per round of every list), the share that adds nothing"""
    d = model.d
    nup = int(np.sum(d["level_nuptrans"]))
    lists = [(int(d["nions"]), int(d["nions"])), (int(d["nalltrans"]), nup), (int(d["nphixstargets_total"]), int(d["nphixstargets_total"])),
             (int(d["nphixstargets_total"]), int(d["nphixstargets_total"])), (int(d["nlevels"]), int(d["nlevels"]))]
    slots = sum(-(-n // 64) * 64 for n, _ in lists)
    return 1.0 - sum(w for _, w in lists) / max(slots, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=10_000_000)
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--model", default="w7")
    ap.add_argument("--host-sample", type=int, default=4096, help="fitted cells the x86 build solves (its time is scaled to all of them); 0: all")
    args = ap.parse_args()
    model, cs, ts, aux = synth.build(args.model, ncoord=args.ncoord)
    model = synth.with_meannucmass(model)
    state = dict(cs.d)
    pk = synth.make_packets(model, aux, args.packets, seed_base=1281360349, kpkt_fraction=0.02, seed=99)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine
    import thermal_common as tc

    eng = engine.Engine(model)
    eng.upload_packets(pk)
    eng.set_cellstate(abi.CellState(state), ts)
    t0 = time.perf_counter()
    eng.step()
    step_ms = (time.perf_counter() - t0) * 1e3
    vol = synth.assocvolume_tmin(model)
    n, g = int(model["npts_nonempty"]), int(model["nbfcontinua_ground"])
    ts_next = tc.next_timestep(model, ts)
    nm = synth.next_matter(model, abi.CellState(state), ts.c.mid, ts_next.c.mid, "classic")
    fit = eng.radfield_fit(ts.c.mid, ts.c.width, vol, lte_iteration=False)
    est = abi.Estimators(n, g)
    eng.download_estimators(est)
    hm = tc.HostModel(model)
    ins = tc.call_inputs(model, state, ts, nm, fit, np.asarray(est.gammaestimator).reshape(n, g).copy(), np.asarray(est.ffheatingestimator).copy(),
                         np.asarray(est.colheatingestimator).copy(), vol)
    # the synthetic heating inputs, sized by every cell's own cooling at its resident T_e (formed on the device: the x86 build would
    # take minutes for it at this size)
    probe = tc.probe_inputs(n, hm.nl)
    matter = dict(rho=nm["rho"], elem_massfracs=nm["elem_massfracs"])
    dep = lambda x: {k: x[k] for k in ("ntlepton_dep", "dep_alpha", "dep_spfission")}  # noqa: E731
    eng.thermal_solve(probe["bfheat"], **matter, **dep(probe))
    r = eng.thermal_rates(probe["bfheat"], Te=np.asarray(state["Te"], np.float32), rebalance=True, **dep(probe))
    ins.update(tc.heating_from_cooling(r["rates"], hm.nl))
    res_rates_ms = r["kernel_ms"]["rates"]
    res = {"cells": n, "packets": args.packets, "step_ms": round(step_ms, 1), "levels": int(model["nlevels"]), "alltrans": int(model["nalltrans"]),
           "phixstargets": int(model["nphixstargets_total"]), "idle_lane_share": round(idle_lane_share(model), 4),
           "rates_all_cells_ms": round(res_rates_ms, 3)}
    wall, kms = [], []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = eng.thermal_solve(ins["bfheat"], rho=nm["rho"], elem_massfracs=nm["elem_massfracs"], ntlepton_dep=ins["ntlepton_dep"],
                              dep_alpha=ins["dep_alpha"], dep_spfission=ins["dep_spfission"])
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(d["kernel_ms"])
    fitted = (fit["flags"] & abi.RADFIELD_FITTED) != 0
    res.update(call_ms=[round(x, 2) for x in wall], renorm_ms=[round(k["renorm"], 3) for k in kms],
               gamma_partfunct_ms=[round(k["gamma_partfunct"], 3) for k in kms], solve_ms=[round(k["solve"], 3) for k in kms],
               fitted=int(d["nfitted"]), flags=d["ncells_flagged"], evals_per_fitted_cell=round(d["total_evals"] / max(int(d["nfitted"]), 1), 2),
               evals_max=int(d["evals"].max(initial=0)))
    # the x86 build of the same rules, on a sample of the fitted cells (evenly spread; the others are handed over as unfitted)
    sample = np.nonzero(fitted)[0]
    if args.host_sample and len(sample) > args.host_sample:
        sample = sample[np.linspace(0, len(sample) - 1, args.host_sample).astype(np.int64)]
    flags_h = np.zeros(n, np.int32)
    flags_h[sample] = abi.RADFIELD_FITTED
    ins_h = dict(ins, fit_flags=flags_h)
    t0 = time.perf_counter()
    h = hm.solve(ins_h, nthreads=args.threads)
    host_ms = (time.perf_counter() - t0) * 1e3
    res.update(host_threads=args.threads, host_sample=int(len(sample)), host_sample_ms=round(host_ms, 1),
               host_ms_scaled=round(host_ms * int(d["nfitted"]) / max(len(sample), 1), 1))
    res["renorm_identical_to_host"] = bool(np.array_equal(d["corrphotoionrenorm"][sample], h["renorm"][sample]))
    both = sample[((d["flags"][sample] & h["flags"][sample]) & abi.THERMAL_BRACKETED) != 0]
    res["worst_Te_rel_to_host"] = float(np.abs(d["Te_solved"][both] / h["Te_solved"][both] - 1).max(initial=0))
    res["cells_Te_identical_to_host"] = round(float((d["Te"][sample] == h["Te"][sample]).mean()) if len(sample) else 1.0, 6)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
