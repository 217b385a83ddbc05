"""The rules of the bound-free heating coefficients (artis_amd/csrc/bf_heating.h) on x86 (tests/bfheat_host): the adaptive 61-point
Gauss-Kronrod integrator against the reference's own (tests/golden/gk61_reference.json: bit for bit, evaluation counts included), the
stage's expm1 against libm's, the coefficient of a constant table against a quadrature that shares neither the integrator nor the
reference, and the renormalisation rules on the synthetic model."""
import math
import os
import subprocess

import numpy as np
import pytest

import bfheat_common as bc
import thermal_common as tc
from artis_amd import abi, synth

fh = float.fromhex


def test_gk61_matches_the_reference_on_analytic_integrands():
    """set (a): result, error estimate and evaluation count bit for bit; the file must hold walks of depth 3 or more and walks that
    reach the 15-level cap, or the walk is untested"""
    gold = bc.golden()["analytic"]
    got = bc.host_gk61(bc.golden_analytic_cases())
    assert len(gold) >= 50
    for c, r in zip(gold, got):
        assert r["result"].hex() == fh(c["result"]).hex() and r["error"].hex() == fh(c["error"]).hex() and r["evals"] == c["evaluations"], (c, r)
        assert r["evals"] == bc.NODE * r["nodes"]
    depths = np.array([r["maxdepth"] for r in got])
    print("walk depths of set (a):", sorted(set(depths.tolist())), "nodes up to", max(r["nodes"] for r in got))
    assert ((depths >= 3) & (depths < bc.MAX_DEPTH)).sum() >= 3 and (depths == bc.MAX_DEPTH).sum() >= 1 and (depths == 0).sum() >= 3
    # a == b gives 0 without an evaluation; b < a negates
    zero = [r for c, r in zip(bc.golden_analytic_cases(), got) if c[2] == c[3]]
    assert len(zero) >= 2 and all(r["result"] == 0.0 and r["evals"] == 0 for r in zero)
    cases = bc.golden_analytic_cases()
    flipped = [(k, c) for k, c in enumerate(cases) if c[3] < c[2]]
    assert len(flipped) >= 3
    back = bc.host_gk61([(w, p, b, a, tol) for _, (w, p, a, b, tol) in flipped])
    for (k, _), r in zip(flipped, back):
        assert got[k]["result"] == -r["result"] and got[k]["error"] == r["error"] and got[k]["evals"] == r["evals"]


def _heating(c):
    xs = np.array(c["xs_bits"], np.uint32).view(np.float32)
    return bc.host_integral(xs, fh(c["increment"]), fh(c["nu_edge"]), fh(c["T_R"]), fh(c["W"]))


def test_heating_integrand_matches_the_reference_integrator():
    """set (b), the stage's own exp and expm1: only the integrator differs, so bit for bit"""
    gold = bc.golden()["heating"]
    assert len(gold) >= 150
    nodes = set()
    for c in gold:
        r = _heating(c)
        assert r["result"].hex() == fh(c["result"]).hex() and r["error"].hex() == fh(c["error"]).hex(), c
        assert r["nodes"] * bc.NODE == c["evaluations"]
        assert math.isfinite(r["result"]) and r["result"] >= 0
        nodes.add(r["nodes"])
    print("nodes per integral of set (b):", sorted(nodes))


def test_heating_integrand_with_libm_within_the_integrators_tolerance():
    """set (b), the same formula on std::exp / std::expm1: both are answers to the integrator's epsrel, 1e-3. The largest difference
    seen is printed (DESIGN.md quotes it)."""
    worst, flips = 0.0, 0
    for c in bc.golden()["heating"]:
        r, ref = _heating(c)["result"], fh(c["result_libm"])
        flips += c["evaluations"] != c["evaluations_libm"]
        if ref == 0.0:
            assert r == 0.0
            continue
        worst = max(worst, abs(r - ref) / abs(ref))
    print(f"own exp / expm1 against libm's over set (b): largest relative difference {worst:.3e}, subdivision decisions flipped: {flips}")
    assert worst <= 1e-3


def test_tb_expm1_against_libm():
    """2 ulp (4.5e-16 relative, the bar tb_exp is held to) over [-700, 709], around 0 down to 1e-300 and at the branch points of
    fdlibm's s_expm1.c; exact at 0, +-inf and NaN"""
    ln2 = math.log(2.0)
    rng = np.random.default_rng(11)
    xs = list(rng.uniform(-700.0, 709.0, 20000)) + list(rng.uniform(-40.0, 40.0, 20000)) + list(rng.uniform(-1.5, 1.5, 20000))
    xs += [s * 10.0 ** e for s in (1.0, -1.0) for e in rng.uniform(-300.0, 0.0, 4000)]
    for b in (0.5 * ln2, 1.5 * ln2, 56 * ln2, 20 * ln2, 19 * ln2, 57 * ln2, 2.0 ** -54, 0.25, 709.782712893384, 1024 * ln2, 1023 * ln2, 2 * ln2, 3 * ln2):
        for s in (1.0, -1.0):
            x = s * b
            xs += [x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf), x * (1 + 1e-9), x * (1 - 1e-9)]
    xs += [700.0, 709.0, -700.0, 1e-300, -1e-300, 5e-324, -5e-324]
    worst, at = 0.0, 0.0
    for x in xs:
        x = float(x)
        try:
            want = math.expm1(x)
        except OverflowError:
            want = math.inf
        got = bc.expm1(x)
        if want == got:
            continue
        assert math.isfinite(want) and math.isfinite(got), (x, got, want)
        rel = abs(got - want) / abs(want)
        if rel > worst:
            worst, at = rel, x
    print(f"tb_expm1 against math.expm1 over {len(xs)} arguments: worst relative difference {worst:.3e} at x = {at!r}")
    assert worst <= 4.5e-16
    assert bc.expm1(0.0) == 0.0 and math.copysign(1.0, bc.expm1(0.0)) == 1.0 and math.copysign(1.0, bc.expm1(-0.0)) == -1.0
    assert bc.expm1(math.inf) == math.inf and bc.expm1(-math.inf) == -1.0 and math.isnan(bc.expm1(math.nan))


@pytest.mark.parametrize("threshold_ev,T_R,W,npoints", [(5.0, 15000.0, 0.3, 12), (13.6, 25000.0, 1e-3, 40), (1.5, 6000.0, 1.0, 100), (24.6, 40000.0, 0.05, 12)])
def test_constant_table_against_a_fine_grid_quadrature(threshold_ev, T_R, W, npoints):
    """A table with all entries equal makes the integrand smooth: 4 pi p sigma W (2h/c^2) int nu^3 (1 - nu_edge/nu) exp(-x) dnu, taken
    here by Simpson's rule on 2e6 intervals (independent of the integrator and of the reference). Bar 1e-8; the parameters keep
    h nu / k T_R below 40 over the range, where one 61-point node integrates the entire function far below the bar."""
    sigma, prob = float(np.float32(3.2e-18)), 0.75
    T_R, W = float(np.float32(T_R)), float(np.float32(W))
    nu_edge = threshold_ev * 1.6021772e-12 / bc.H
    r = bc.host_integral(np.full(npoints, sigma, np.float32), 0.1, nu_edge, T_R, W)
    got = r["result"] * (4 * math.pi * prob)
    want = bc.closed_form(sigma, prob, nu_edge, nu_edge * (1.0 + 0.1 * (npoints - 1)), T_R, W)
    print(f"{threshold_ev} eV, {T_R} K, {npoints} points: {got!r} against {want!r}, relative difference {abs(got - want) / want:.3e}, nodes {r['nodes']}")
    assert bc.H * nu_edge * (1.0 + 0.1 * (npoints - 1)) / bc.KB / T_R < 40
    assert abs(got - want) <= 1e-8 * want


class Case:
    """the synthetic model with a thick core, a synthetic fit whose T_R and W differ from the resident ones, and raw estimators"""

    def __init__(self, gridtype=abi.GRID_CARTESIAN3D):
        self.model, cs, self.ts, aux = tc.build_model(gridtype)
        self.state = dict(cs.d)
        self.hm = bc.HostModel(self.model)
        n, g = self.hm.n, self.hm.g
        rng = np.random.default_rng(7)
        self.vol = synth.assocvolume_tmin(self.model)
        self.fitted = np.asarray(self.state["thick"]) != tc.CELL_THICK
        self.fit = dict(TR=np.asarray(self.state["TR"], np.float32) * np.float32(1.1), W=np.asarray(self.state["W"], np.float32) * np.float32(0.8),
                        flags=self.fitted.astype(np.int32) * abi.RADFIELD_FITTED)
        self.enf = 1 / (np.asarray(self.vol, np.float64) * (self.ts.c.mid / float(self.model["tmin"])) ** 3) / self.ts.c.width
        self.bfh_raw = 10.0 ** rng.uniform(-14, -10, (n, g)) / self.enf[:, None]
        self.ins = bc.call_inputs(self.model, self.state, self.ts, self.fit, self.bfh_raw, self.vol)
        self.out = self.hm.update(self.ins)
        d = self.model.d
        self.start = np.asarray(d["ion_uniquelevelindexstart"])
        self.level_ion = np.searchsorted(self.start, np.arange(self.hm.nl), side="right") - 1

    def target_integral(self, ul, t, T_R, W):
        """(the integral of target t of level ul by the x86 integrator, its probability): table, threshold and probability looked up here"""
        d = self.model.d
        k = int(d["level_phixstargetstart"][ul]) + t
        upper = int(self.start[self.level_ion[ul] + 1]) + int(d["allphixstargets_levelindex"][k])
        nu_edge = (1.0 / bc.H) * (float(d["level_epsilon"][upper]) - float(d["level_epsilon"][ul]))
        NP = int(d["NPHIXSPOINTS"])
        xs = np.asarray(d["allphixs"], np.float32)[int(d["level_phixsstart"][ul]) * NP:][:NP]
        return bc.host_integral(xs, float(d["NPHIXSNUINCREMENT"]), nu_edge, float(T_R), float(W))["result"], float(d["allphixstargets_probability"][k])


@pytest.fixture(scope="module")
def case():
    return Case()


def test_unfitted_rows_are_zero_and_fitted_ones_positive(case):
    o, fitted = case.out, case.fitted
    assert 0 < fitted.sum() < case.hm.n
    assert not o["coeffs"][~fitted].any() and not np.signbit(o["coeffs"][~fitted]).any()
    assert not o["renorm"][~fitted].any() and not o["flags"][~fitted].any()
    nt = np.asarray(case.model.d["level_nphixstargets"])
    assert not o["coeffs"][:, nt == 0].any() and not np.signbit(o["coeffs"][:, nt == 0]).any()
    assert np.isfinite(o["coeffs"]).all() and (o["coeffs"][fitted][:, nt > 0] > 0).all() and o["nonfinite"] == 0
    gci = case.hm.gci()
    nground = int((gci >= 0).sum())
    assert o["totals"]["nodes"] == int(fitted.sum()) * (int(nt.sum()) + nground)  # one node per integral
    assert o["totals"]["subdivided"] == 0 and o["totals"]["at_depth_cap"] == 0


def test_ground_reads_the_resident_field_and_levels_the_fits(case):
    """renorm = estimator x normfactor / (4 pi p x the ground integral in the RESIDENT T_R, W); a level's coefficient = the sum of its
    targets' integrals in the FIT's T_R, W, in index order from 0., times the factor of its closest ground continuum. Both rebuilt here
    from per-target integrals, bit for bit; the two fields differ by 10 and 20 per cent."""
    d, o = case.model.d, case.out
    gci = case.hm.gci()
    nt = np.asarray(d["level_nphixstargets"])
    closest = np.asarray(d["level_closestgroundlevelcont"])
    cells = np.nonzero(case.fitted)[0][[0, -1]]
    two, none = 0, 0
    for c in cells:
        rTR, rW = case.state["TR"][c], case.state["W"][c]
        fTR, fW = case.fit["TR"][c], case.fit["W"][c]
        assert rTR != fTR and rW != fW
        for ui in np.nonzero(gci >= 0)[0]:
            integral, p = case.target_integral(int(case.start[ui]), 0, rTR, rW)
            ground = integral * (4 * math.pi * p)
            normed = case.bfh_raw[c, gci[ui]] * (1 / (case.vol[c] * (case.ts.c.mid / float(d["tmin"])) ** 3) / case.ts.c.width / 1)
            assert o["renorm"][c, gci[ui]] == normed / ground, (c, ui)
        for ul in np.nonzero(nt > 0)[0]:
            s = 0.0
            for t in range(nt[ul]):
                integral, p = case.target_integral(int(ul), t, fTR, fW)
                s += integral * (4 * math.pi * p)
            if closest[ul] >= 0:
                s *= o["renorm"][c, closest[ul]]
            else:
                none += 1
            two += nt[ul] >= 2
            assert o["coeffs"][c, ul] == s, (c, ul)
    print(f"levels rebuilt: {len(cells) * int((nt > 0).sum())}, with two or more targets {two}, without a ground continuum {none}")
    assert two > 0


def test_no_ground_continuum_means_no_factor(case):
    """doubling the estimators doubles exactly the coefficients of the levels with a closest ground continuum and no other"""
    closest = np.asarray(case.model.d["level_closestgroundlevelcont"])
    twice = case.hm.update(dict(case.ins, bfh_raw=2.0 * case.bfh_raw))
    assert np.array_equal(twice["coeffs"][:, closest >= 0], 2.0 * case.out["coeffs"][:, closest >= 0])
    assert np.array_equal(twice["coeffs"][:, closest < 0], case.out["coeffs"][:, closest < 0])
    # and the levels' field does not reach the factors, nor the resident one the raw sums
    other = case.hm.update(dict(case.ins, lev_TR=case.fit["TR"] * np.float32(1.3)))
    assert np.array_equal(other["renorm"], case.out["renorm"]) and not np.array_equal(other["coeffs"], case.out["coeffs"])


def test_zero_ground_integral_gives_factor_one_and_the_flag(case):
    """an integral that is not > 0 (W = 0; T_R = MINTEMP under a threshold high enough to underflow) cannot renormalise: factor 1, flag"""
    mintemp = tc.lib().tb_host_mintemp()
    high = bc.host_integral(np.full(12, 1e-18, np.float32), 0.1, 1200 * bc.KB * mintemp / bc.H, mintemp, 1.0)
    assert high["result"] == 0.0 and high["nodes"] == 1  # (h nu / k T_R >= 1200: 1 / expm1 underflows, the Planck function is 0)
    cells = np.nonzero(case.fitted)[0][:3]
    TR, W = np.array(case.state["TR"], np.float32), np.array(case.state["W"], np.float32)
    W[cells[0]] = 0.0
    TR[cells[1]] = mintemp
    o = case.hm.update(dict(case.ins, res_TR=TR, res_W=W))
    gci = case.hm.gci()
    has = np.zeros(case.hm.g, bool)
    has[gci[gci >= 0]] = True
    assert (o["renorm"][cells[0]][has] == 1.0).all() and o["flags"][cells[0]] & abi.BFHEAT_RENORM_ONE
    one = o["renorm"][cells[1]][has] == 1.0  # at MINTEMP: exactly the continua whose integral underflowed
    assert bool(o["flags"][cells[1]] & abi.BFHEAT_RENORM_ONE) == bool(one.any())
    for ui in np.nonzero(gci >= 0)[0]:
        integral, _ = case.target_integral(int(case.start[ui]), 0, mintemp, W[cells[1]])
        assert (integral > 0) != (o["renorm"][cells[1], gci[ui]] == 1.0), ui
    assert not o["flags"][cells[2]] and np.isfinite(o["coeffs"]).all()
    assert np.array_equal(o["coeffs"][cells[2]], case.out["coeffs"][cells[2]])


def test_edge_fields_stay_finite(case):
    """the levels' integrals at W = 0, T_R = MINTEMP and T_R = MAXTEMP (small expm1 arguments): finite, W = 0 gives +0"""
    L = tc.lib()
    cells = np.nonzero(case.fitted)[0][:3]
    TR, W = np.array(case.fit["TR"], np.float32), np.array(case.fit["W"], np.float32)
    W[cells[0]] = 0.0
    TR[cells[1]], TR[cells[2]] = L.tb_host_mintemp(), L.tb_host_maxtemp()
    o = case.hm.update(dict(case.ins, lev_TR=TR, lev_W=W))
    assert np.isfinite(o["coeffs"]).all() and o["nonfinite"] == 0 and (o["coeffs"] >= 0).all()
    assert not o["coeffs"][cells[0]].any()
    nt = np.asarray(case.model.d["level_nphixstargets"])
    assert (o["coeffs"][cells[2]][nt > 0] > 0).all()


def test_two_calls_and_thread_counts_identical(case):
    a, b = case.hm.update(case.ins, nthreads=1), case.hm.update(case.ins, nthreads=7)
    for k in ("coeffs", "renorm", "flags"):
        assert a[k].tobytes() == b[k].tobytes() == case.out[k].tobytes(), k
    assert a["totals"] == b["totals"] == case.out["totals"]


def test_unsupported_build_says_so():
    assert bc.lib("classic").bfh_host_supported() == 1 and bc.lib("kilonova_lte").bfh_host_supported() == 0


def test_harness_under_the_sanitizers(case, tmp_path):
    """tests/bfheat_host/rows_main.cc, a program of its own built with -fsanitize=address,undefined: the threaded update on the 3D case and
    on a 1D one, every array in an allocation of exactly its size, and the walk down to its depth cap; its counts are the library's"""
    subprocess.check_call(["make", "-C", bc.HOSTDIR, "rows_sanitized"], stdout=subprocess.DEVNULL)
    cases = [case, Case(abi.GRID_SPHERICAL1D)]
    paths = []
    for k, cs in enumerate(cases):
        paths.append(str(tmp_path / f"call{k}.bin"))
        bc.dump_call(cs.hm, cs.ins, paths[-1])
    out = subprocess.run([os.path.join(bc.HOSTDIR, "rows_sanitized")] + paths, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 2
    for cs, line in zip(cases, lines):
        t = cs.out["totals"]
        want = f"{cs.hm.n} cells, {int((cs.out['flags'] != 0).sum())} flagged, {t['nodes']} nodes, {t['subdivided']} integrals subdivided, {t['at_depth_cap']} at the cap"
        assert want in line and f"to depth {bc.MAX_DEPTH}" in line, (want, line)
