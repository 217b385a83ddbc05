"""Regenerate tests/golden/gk61_reference.json from the REFERENCE's own gausskronrod.h.

    python tests/golden/make_gk61_golden.py <reference source tree>

Needs the reference's source tree. gk61_golden.cc includes its gausskronrod.h where it lies (nothing of it is copied) and the project's
artis_amd/csrc/bf_heating.h for the integrands, so that only the integrator differs: the reference's
gauss_kronrod_integrate<61>(f, a, b, 15, tol, &error) on
  (a) analytic integrands built from + - * / and sqrt only (artis_bfh::Gk61TestFn) on intervals of order 1: polynomials, 1/(1+x^2),
      sqrt(x), |x - 0.3|, a step at an irrational point, ..., at tolerances from 1e-3 down to 1e-14, so that some subdivide a few levels
      and the step runs into the 15-level cap; a == b and b < a among them;
  (b) the project's own bound-free heating integrand (artis_bfh::BfhIntegrand) on seeded step-function tables of 12 / 40 / 100 points,
      thresholds of 1.5 - 50 eV, T_R of 1000 - 100 000 K and W of 1e-6 - 1, each twice: with the stage's own exp / expm1 and with libm's.
Stores results and error estimates as hex floats, the tables as the bit patterns of their floats, and the evaluation counts.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
H, EV = 6.6260755e-27, 1.6021772e-12
SQRT_HALF, GOLDEN = 0.7071067811865476, 0.6180339887498949


def analytic_cases():
    cases = []
    tols = (1e-3, 1e-6, 1e-9, 1e-12, 1e-14)
    for tol in tols:
        cases += [(0, 2.0, 0.0, 1.0, tol), (0, -0.5, -1.0, 2.0, tol), (1, 1.0, 0.0, 1.0, tol), (1, 1.0, -3.0, 4.0, tol), (1, 25.0, -1.0, 1.0, tol),
                  (2, 0.0, 0.0, 1.0, tol), (2, 0.0, 0.25, 2.0, tol), (3, 0.3, 0.0, 1.0, tol), (3, 0.3, -1.0, 0.5, tol),
                  (4, SQRT_HALF, 0.0, 1.0, tol), (4, GOLDEN, 0.5, 1.5, tol), (5, 3.0, -1.0, 1.0, tol), (5, 0.5, 0.0, 1.5, tol),
                  (6, 1e-6, 0.0, 1.0, tol), (7, 0.3, 0.0, 1.0, tol), (7, SQRT_HALF, 0.0, 2.0, tol)]
    for tol in (1e-4, 1e-5, 1e-7, 1e-8):  # walks that end between depth 1 and depth 9
        cases += [(6, 1e-2, 0.0, 1.0, tol), (6, 1e-3, 0.0, 1.0, tol), (6, 1e-4, 0.0, 1.0, tol), (1, 400.0, -1.0, 1.0, tol), (1, 1e4, -1.0, 1.0, tol),
                  (3, 0.3, 0.0, 1.0, tol)]
    cases += [(0, 2.0, 1.0, 1.0, 1e-3), (1, 1.0, 0.5, 0.5, 1e-9), (3, 0.3, 1.0, 0.0, 1e-6), (1, 1.0, 2.0, -1.0, 1e-9), (4, SQRT_HALF, 1.0, 0.0, 1e-12),
              (2, 0.0, 1.0, 0.0, 1e-12)]
    return cases


def bfh_cases(rng):
    cases = []
    for npoints, count in ((12, 130), (40, 50), (100, 20)):
        for k in range(count):
            nu_edge = float(rng.uniform(1.5, 50.0)) * EV / H
            if k % 10 == 0:
                T_R = (1000.0, 100000.0, 500.0)[(k // 10) % 3]
            else:
                T_R = float(np.exp(rng.uniform(np.log(3000.0), np.log(40000.0))))
            W = float(10.0 ** rng.uniform(-6, 0))
            x = 1.0 + 0.1 * np.arange(npoints)
            if k % 7 == 3:
                xs = np.full(npoints, 10.0 ** rng.uniform(-19, -17))
            else:
                xs = 10.0 ** rng.uniform(-19, -17) * x ** -rng.uniform(1.0, 4.0) * 10.0 ** rng.uniform(-0.3, 0.3, npoints)
                if k % 7 == 5:
                    xs[rng.integers(0, npoints, npoints // 3)] = 0.0  # gaps in the table
            cases.append((npoints, 0.1, nu_edge, float(np.float32(T_R)), float(np.float32(W)), xs.astype(np.float32)))
    return cases


def main():
    reference = sys.argv[1]
    rng = np.random.default_rng(61)
    fn, bfh = analytic_cases(), bfh_cases(rng)
    lines = [f"fn {w} {float(p).hex()} {float(a).hex()} {float(b).hex()} {float(tol).hex()}" for w, p, a, b, tol in fn]
    lines += [f"bfh {n} {inc.hex()} {nu.hex()} {T.hex()} {W.hex()} " + " ".join(float(v).hex() for v in xs) for n, inc, nu, T, W, xs in bfh]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gk61_golden")
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-fno-fast-math", "-I", reference, "-o", exe,
                               os.path.join(HERE, "gk61_golden.cc"), "-lm"])
        res = subprocess.run([exe], input="\n".join(lines) + "\n", text=True, capture_output=True, check=True).stdout.split("\n")
    analytic, heating = [], []
    for (w, p, a, b, tol), line in zip(fn, res):
        r, e, n = line.split()
        analytic.append(dict(which=w, p=float(p).hex(), a=float(a).hex(), b=float(b).hex(), tol=float(tol).hex(), result=float.fromhex(r).hex(),
                             error=float.fromhex(e).hex(), evaluations=int(n)))
    for (n, inc, nu, T, W, xs), line in zip(bfh, res[len(fn):]):
        r, e, k, rl, el, kl = line.split()
        heating.append(dict(npoints=n, increment=inc.hex(), nu_edge=nu.hex(), T_R=T.hex(), W=W.hex(), xs_bits=[int(v) for v in xs.view(np.uint32)],
                            result=float.fromhex(r).hex(), error=float.fromhex(e).hex(), evaluations=int(k),
                            result_libm=float.fromhex(rl).hex(), error_libm=float.fromhex(el).hex(), evaluations_libm=int(kl)))
    out = {"call": "gauss_kronrod_integrate<61>(f, a, b, 15, tol, &error) of the reference's gausskronrod.h",
           "functions": {"0": "1 + x(p + x^2)", "1": "1/(1 + p x^2)", "2": "sqrt(x)", "3": "|x - p|", "4": "x < p ? 1 : 2", "5": "x^10 - p x^5 + x",
                         "6": "1/sqrt(x + p)", "7": "x < p ? 0 : sqrt(x - p)"},
           "integrand": "artis_bfh::BfhIntegrand (artis_amd/csrc/bf_heating.h) over [nu_edge, nu_edge (1 + increment (npoints - 1))], tol 1e-3; "
                        "result/error/evaluations with tb_exp and tb_expm1, *_libm with std::exp and std::expm1; xs_bits: the table's floats",
           "analytic": analytic, "heating": heating}
    with open(os.path.join(HERE, "gk61_reference.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote gk61_reference.json with", len(analytic), "analytic and", len(heating), "heating cases")


if __name__ == "__main__":
    main()
