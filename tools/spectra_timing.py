#!/usr/bin/env python3
"""Cost of the device binning (artis_amd_spectra_compute) at bench scale: the bench model (w7, 50^3 cells, 1e7 packets) after
5 resident timesteps, then wall time of dirbin -1, dirbin -1 with emission / absorption, and all direction bins, the device memory
the binning keeps, and the escaped count. One JSON line.

    python tools/spectra_timing.py [--packets 10000000] [--steps 5] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from artis_amd import abi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=10_000_000)
    ap.add_argument("--ncoord", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    model, cs0, _, aux = synth.build("w7", ncoord=args.ncoord, nts=10)
    pk = synth.make_packets(model, aux, args.packets, seed_base=1281360349, kpkt_fraction=0.02, seed=99,
                            ts_width_frac=1.05 ** args.steps - 1.0)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    from artis_amd import engine

    eng = engine.Engine(model)
    eng.upload_packets(pk)
    t, starts, widths, step_ms = aux["t"], [], [], []
    for i in range(args.steps):
        ts = synth.make_timestep(t, width_frac=0.05, vmax=model["vmax"], nts=10 + i)
        eng.set_cellstate(synth.evolve_cellstate(cs0, aux["t"], ts.c.mid), ts)
        t0 = time.perf_counter()
        eng.step()
        step_ms.append((time.perf_counter() - t0) * 1e3)
        starts.append(ts.c.start)
        widths.append(ts.c.width)
        t = ts.c.start + ts.c.width
    starts, widths = np.array(starts), np.array(widths)
    free0 = torch.cuda.mem_get_info()[0]
    res = {"packets": args.packets, "steps": args.steps, "step_ms": [round(x, 1) for x in step_ms]}
    for name, kw in (("dirbin-1", {}), ("dirbin-1_emission_absorption", dict(emission_absorption=True)),
                     ("all_dirbins", dict(dirbin=abi.SPEC_ALL_DIRBINS))):
        ms = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            eng.spectra_compute(starts, widths, starts[0] * 0.999, t, **kw)
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name + "_ms"] = [round(x, 2) for x in ms]
        res[name + "_extra_mb"] = round((free0 - torch.cuda.mem_get_info()[0]) / 2**20, 1)
    d = eng.spectra_download()
    res["nescaped_rpkt"], res["nescaped_gamma"] = d["nescaped"], d["nescaped_gamma"]
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
