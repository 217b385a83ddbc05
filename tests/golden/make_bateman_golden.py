"""Writes tests/golden/bateman_reference.json: the Bateman sum of every decay path of synth.decay_network("small") at the six times of
tests/decay_common.py, in 80-digit arithmetic (mpmath), from the same double-precision decay constants the engine uses (1 / mean life,
rounded once). "exact" is the chain-end abundance per unit initial abundance of the top; "exact_sink" (alpha-terminated paths) the same with the
last decay constant zeroed, which is the He4 coefficient's sum. Values are decimal strings of 25 digits.

    python tests/golden/make_bateman_golden.py
"""
import json
import os
import sys

import mpmath

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

import decay_common as dc  # noqa: E402
from artis_amd import abi, synth  # noqa: E402

mpmath.mp.dps = 80


def bateman(lambdas, t):
    lam = [mpmath.mpf(float(x)) for x in lambdas]
    t = mpmath.mpf(float(t))
    total = mpmath.mpf(0)
    for j, lj in enumerate(lam):
        den = mpmath.mpf(1)
        for p, lp in enumerate(lam):
            if p != j:
                den *= lp - lj
        total += mpmath.exp(-lj * t) / den
    prod = mpmath.mpf(1)
    for lj in lam[:-1]:
        prod *= lj
    return prod * total


def main():
    net = synth.decay_network("small")
    paths = []
    for p in range(len(net["path_start"]) - 1):
        lam = dc.path_lambdas(net, p)
        entry = dict(nucindex=[int(i) for i in net["path_nucindex"][net["path_start"][p]: net["path_start"][p + 1]]],
                     lambdas_hex=[float(x).hex() for x in lam],
                     exact=[mpmath.nstr(bateman(lam, d * dc.DAY), 25) for d in dc.TIMES_DAYS], exact_sink=None)
        if net["path_last_decaytype"][p] == abi.DECAYTYPE_ALPHA:
            sink = list(lam[:-1]) + [0.0]
            entry["exact_sink"] = [mpmath.nstr(bateman(sink, d * dc.DAY), 25) for d in dc.TIMES_DAYS]
        paths.append(entry)
    out = dict(mpmath=mpmath.__version__, digits=mpmath.mp.dps, times_days=list(dc.TIMES_DAYS), paths=paths)
    with open(os.path.join(HERE, "bateman_reference.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
