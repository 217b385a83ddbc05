"""The rules of artis_amd/csrc/ratecoeff_tables.h (precalculate_rate_coefficient_integrals, ratecoeff.cc:143-233) on x86
(tests/ratecoeff_host): the libm build against a Python restatement of the reference bit for bit, the shared-node form against three
independent integrals, the stage's own exp / expm1 against libm's, closed forms on a flat table, the layout, the node count, and the
harness under the sanitizers."""
import decimal
import math
import os
import subprocess

import numpy as np
import pytest

import ratecoeff_common as rc
from artis_amd import synth

# constants.h
H, KB, CLIGHT, SAHACONST, PI = 6.6260755e-27, 1.38064852e-16, 2.99792458e10, 2.0706659e-16, 3.14159265358979323846
CLIGHTSQUARED = CLIGHT * CLIGHT
HOVERKB = H / KB
FOURPI = 4 * PI
EPSREL = 1e-3
PRESETS = ("classic", "kilonova_lte")
INTERPOLATED = {"classic": False, "kilonova_lte": True, "nltenebular": True}  # PHIXS_CLASSIC_NO_INTERPOLATION == 0


def f32(x) -> float:
    return float(np.float32(x))


def c_expm1(x: float) -> float:
    """glibc's expm1 as C sees it: +inf where Python's wrapper raises for the overflow"""
    try:
        return math.expm1(x)
    except OverflowError:
        return math.inf


# ---------------------------------------------------------------- the reference, restated
class Restated:
    """ratecoeff.cc:75-233 and gausskronrod.h:173-257 in scalar Python floats (IEEE doubles, glibc's exp / expm1 / pow through math)"""

    def __init__(self, model, preset):
        self.m, self.interp = model, INTERPOLATED[preset]
        tablesize, mintemp, maxtemp = synth.OPTION_TABLES[preset]
        step = (math.log(maxtemp) - math.log(mintemp)) / (tablesize - 1.0)  # ratecoeff.cc:39
        self.tgrid = [mintemp * math.exp(i * step) for i in range(tablesize)]
        self.NP, self.INC = int(model["NPHIXSPOINTS"]), float(model["NPHIXSNUINCREMENT"])
        self.last = 1.0 + (self.INC * (self.NP - 1))
        self.gx, self.gw, self.gwg = (a.tolist() for a in rc.gk61_tables(preset))
        self.nodes = 0

    def sigma(self, xs, nu_edge, nu):  # photoionisation_crosssection_fromtable atomic.h:202
        NP, INC = self.NP, self.INC
        if not self.interp:
            if nu < nu_edge:
                return 0.0
            if nu == nu_edge:
                return float(xs[0])
            if nu < nu_edge * (1 + (INC * NP)):
                return float(xs[min(int((nu - nu_edge) / (INC * nu_edge)), NP - 1)])
            return f32(float(xs[NP - 1]) * math.pow(nu_edge * (1 + (INC * NP)) / nu, 3))
        ireal = ((nu / nu_edge) - 1.0) / INC
        i = int(math.floor(ireal))
        if i < 0:
            return 0.0
        if i < NP - 1:
            a, b, fb = float(xs[i]), float(xs[i + 1]), ireal - i
            return f32(((1.0 - fb) * a) + (fb * b))
        r = (nu_edge * self.last) / nu
        return f32(float(xs[NP - 1]) * (r * r * r))

    def unit(self, f, scale, mean):  # integrate_non_adaptive_m1_1<61>
        x, w, wg = self.gx, self.gw, self.gwg
        kr = f((scale * 0.0) + mean) * w[0]
        gr = 0.0
        for i in range(1, 31, 2):
            s = f((scale * x[i]) + mean) + f((scale * -x[i]) + mean)
            kr += s * w[i]
            gr += s * wg[i // 2]
        for i in range(2, 31, 2):
            s = f((scale * x[i]) + mean) + f((scale * -x[i]) + mean)
            kr += s * w[i]
        self.nodes += 1
        return kr, max(abs(kr - gr), abs(kr * 2.220446049250313e-16 * 2))

    def adaptive(self, f, a, b, levels, abs_tol):  # recursive_adaptive_integrate<61>
        mean, scale = (b + a) / 2, (b - a) / 2
        r1, err = self.unit(f, scale, mean)
        estimate = scale * r1
        abs_tol1 = abs(estimate * EPSREL)
        if abs_tol == 0:
            abs_tol = abs_tol1
        if levels != 0 and abs_tol1 < err and abs_tol < err:
            mid = (a + b) / 2
            return self.adaptive(f, a, mid, levels - 1, abs_tol / 2) + self.adaptive(f, mid, b, levels - 1, abs_tol / 2)
        return estimate

    def integrate(self, f, a, b):
        return self.adaptive(f, a, b, 15, 0.0)

    def consts(self, ul, t):
        m = self.m
        ui = int(np.searchsorted(np.asarray(m["ion_uniquelevelindexstart"]), ul, side="right")) - 1
        ts = int(m["level_phixstargetstart"][ul]) + t
        upper = int(m["ion_uniquelevelindexstart"][ui + 1]) + int(m["allphixstargets_levelindex"][ts])
        E_threshold = float(m["level_epsilon"][upper]) - float(m["level_epsilon"][ul])
        nu_threshold = E_threshold / H
        start = int(m["level_phixsstart"][ul]) * self.NP
        return dict(g_lower=float(m["level_statweight"][ul]), g_upper=float(m["level_statweight"][upper]),
                    prob=float(m["allphixstargets_probability"][ts]), nu_threshold=nu_threshold, nu_max=nu_threshold * self.last,
                    xs=np.asarray(m["allphixs"])[start:start + self.NP])

    def entry(self, ul, t, ti, lut_photoion=True):
        k = self.consts(ul, t)
        nu_edge, xs = k["nu_threshold"], k["xs"]
        T = f32(self.tgrid[ti])
        sahafact = SAHACONST * k["g_lower"] / k["g_upper"] * math.pow(T, -1.5)

        def alpha(x):
            return (2 / CLIGHTSQUARED) * self.sigma(xs, nu_edge, x + nu_edge) * ((nu_edge + x) * (nu_edge + x)) * math.exp(-HOVERKB * x / T)

        def gammacorr(nu):
            planck = 2 * H * (nu * nu * nu) / (CLIGHT * CLIGHT) / c_expm1(HOVERKB * nu / T)
            return self.sigma(xs, nu_edge, nu) * (1.0 / H) / nu * planck * (1 - math.exp(-HOVERKB * nu / T))

        def cooling(x):
            return self.sigma(xs, nu_edge, x + nu_edge) * x * (2 * H / CLIGHTSQUARED) * (x + nu_edge) * (x + nu_edge) * math.exp(-HOVERKB * x / T)

        out = [FOURPI * sahafact * k["prob"] * self.integrate(alpha, 0, k["nu_max"] - nu_edge), None, None]
        if lut_photoion:
            out[1] = self.integrate(gammacorr, nu_edge, k["nu_max"]) * (FOURPI * k["prob"])
        out[2] = FOURPI * sahafact * k["prob"] * self.integrate(cooling, 0, k["nu_max"] - nu_edge)
        return out


_CASES = {}


def _case(preset):
    """the small model of a preset, the x86 build's view of it and its tables in both Math policies (made once, never changed)"""
    if preset not in _CASES:
        m = rc.model(preset)
        hm = rc.HostModel(m, preset)
        _CASES[preset] = dict(preset=preset, model=m, hm=hm, libm=hm.tables(rc.LIBM, shared=False), tb=hm.tables(rc.TBMATH, shared=True))
    return _CASES[preset]


@pytest.fixture(scope="module", params=PRESETS)
def case(request):
    return _case(request.param)


def test_libm_build_matches_the_reference_restated(case):
    """every continuum at the temperature indices 0, last and every 7th: all three tables bit for bit; the grid and Tpow too"""
    hm, got = case["hm"], case["libm"]
    ref = Restated(case["model"], case["preset"])
    assert hm.tgrid.tolist() == ref.tgrid
    assert hm.Tpow.tolist() == [math.pow(f32(T), -1.5) for T in ref.tgrid]
    tis = sorted(set(range(0, hm.tablesize, 7)) | {0, hm.tablesize - 1})
    assert hm.ncovered == hm.nbf > 100
    nchecked = 0
    for ci, (ul, t) in enumerate(hm.conts):
        for ti in tis:
            want = ref.entry(int(ul), int(t), ti)
            have = [got[k][ci, ti] for k in rc.TABLES]
            assert [float(v).hex() for v in have] == [float(v).hex() for v in want], (ci, ul, t, ti, have, want)
            nchecked += 3
    assert ref.nodes == nchecked  # the restated walk too ends after every first node


def test_shared_nodes_equal_independent_integrals(case):
    """alpha_sp and bfcooling from one set of evaluations (the kernel's form) against three gk61_integrate calls per entry: every entry
    of every table, the flags and the totals, in both Math policies"""
    hm = case["hm"]
    for math_policy, independent, shared in ((rc.LIBM, case["libm"], hm.tables(rc.LIBM, shared=True)),
                                             (rc.TBMATH, hm.tables(rc.TBMATH, shared=False), case["tb"])):
        rc.same_tables(shared, independent, (case["preset"], math_policy))
        assert shared["totals"] == independent["totals"]


# the largest relative difference between the TbMath and the libm build, measured on the two models of this file (the per-table
# figures are printed below and recorded in DESIGN.md, "Rate-coefficient tables"); the bar is four times it, the project's rule where
# no ulp table of the device's functions exists
MEASURED_TB_VS_LIBM = {"spontrecombcoeffs": 5.71e-16, "corrphotoioncoeffs": 4.49e-16, "bfcooling_coeffs": 5.92e-16}


TINY = 1e-280  # below it an entry's terms reach the subnormals (gammacorr at 500 K under a 30 eV edge underflows to +0)


def _relative(a, b) -> float:
    """the largest |a - b| / b over the entries with b above TINY; at and below TINY the two must agree to TINY's own last bits"""
    big = b > TINY
    assert (b >= 0).all() and np.all(np.abs(a[~big] - b[~big]) <= TINY * 2.2e-16)
    return float(np.max(np.abs(a[big] - b[big]) / b[big]))


def test_tbmath_against_libm(case):
    tb, libm = case["tb"], case["libm"]
    for k in rc.TABLES:
        rel = _relative(tb[k], libm[k])
        print(f"{case['preset']} {k}: TbMath against libm, largest relative difference {rel:.3e}")
        assert rel <= 4 * MEASURED_TB_VS_LIBM[k], (k, rel)
    # alpha_sp and bfcooling are sums of 61 non-negative terms: a few ulp of exp (tb_exp: below 1 ulp; libm: below 1) plus the
    # roundings of a term and of the running sums cannot exceed (2 + 4 + 61) ulp even if all went one way
    for k in ("spontrecombcoeffs", "bfcooling_coeffs"):
        assert (libm[k] > TINY).all() and _relative(tb[k], libm[k]) < 67 * 2.2e-16
    assert tb["flags"].tobytes() == libm["flags"].tobytes() and tb["totals"] == libm["totals"]


def _closed_forms(nu0: float, L: float, a: float, sigma: float):
    """(2/c^2) sigma int_0^L (nu0 + x)^2 e^{-ax} dx and sigma (2h/c^2) int_0^L x (nu0 + x)^2 e^{-ax} dx from
    I_n = int_0^L x^n e^{-ax} dx = n!/a^(n+1) (1 - e^{-aL} sum_{k<=n} (aL)^k / k!), in 60 decimal digits"""
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        nu0, L, a, sigma = D(nu0), D(L), D(a), D(sigma)
        eaL = (-a * L).exp()
        In = []
        for n in range(4):
            partial = sum(((a * L) ** k) / math.factorial(k) for k in range(n + 1))
            In.append(D(math.factorial(n)) / a ** (n + 1) * (1 - eaL * partial))
        c2 = D(CLIGHT) * D(CLIGHT)
        alpha = (2 / c2) * sigma * (nu0 * nu0 * In[0] + 2 * nu0 * In[1] + In[2])
        cooling = sigma * (2 * D(H) / c2) * (nu0 * nu0 * In[1] + 2 * nu0 * In[2] + In[3])
        return alpha, cooling


def test_flat_table_against_closed_forms():
    """every cross-section point 6e-18f (classic form: no interpolation): the integrands are polynomials times an exponential. Entries
    with h L / k T <= 120 (L: the interval's length) are held to 1e-12; above that the single 61-point node itself degrades, and the
    condition, not the error, excludes them."""
    m = rc.model("classic")
    flat = rc.changed(m, allphixs=np.full(len(m["allphixs"]), 6e-18, np.float32))
    hm = rc.HostModel(flat, "classic")
    ref = Restated(flat, "classic")
    sigma = f32(6e-18)
    worst, nheld, nexcluded = 0.0, 0, 0
    for math_policy in (rc.LIBM, rc.TBMATH):
        got = hm.tables(math_policy, shared=True)
        for ci, (ul, t) in enumerate(hm.conts):
            k = ref.consts(int(ul), int(t))
            L = k["nu_max"] - k["nu_threshold"]
            for ti in range(hm.tablesize):
                T = f32(hm.tgrid[ti])
                a = HOVERKB / T
                if a * L > 120:
                    nexcluded += 1
                    continue
                alpha, cooling = _closed_forms(k["nu_threshold"], L, a, sigma)
                pre = FOURPI * (SAHACONST * k["g_lower"] / k["g_upper"] * hm.Tpow[ti]) * k["prob"]
                for name, exact in (("spontrecombcoeffs", alpha), ("bfcooling_coeffs", cooling)):
                    want = decimal.Decimal(pre) * exact
                    rel = abs(float((decimal.Decimal(float(got[name][ci, ti])) - want) / want))
                    worst = max(worst, rel)
                    assert rel <= 1e-12, (math_policy, name, ci, ti, rel, a * L)
                nheld += 1
    print(f"flat table: {nheld} entries held (largest relative error {worst:.2e}), {nexcluded} above h L / k T = 120")
    assert nheld > 1000


def test_layout_and_uncovered_rows():
    """continuum-major rows at level_bflist_start[level] + target; a level with two targets has two adjacent rows; the rows of an ion
    with nlevels_ionising = 0 (the test's own copy of the model: every ion of the small model ionises) are +0.0 in every table"""
    m = rc.model("classic")
    nt, start = np.asarray(m["level_nphixstargets"]), np.asarray(m["level_bflist_start"])
    assert (nt == 2).any()
    ionising = np.array(m["ion_nlevels_ionising"])
    ui = int(np.nonzero(ionising > 0)[0][1])
    ionising[ui] = 0
    cut = rc.changed(m, ion_nlevels_ionising=ionising)
    hm, full = rc.HostModel(cut, "classic"), rc.HostModel(m, "classic")
    lo, hi = int(m["ion_uniquelevelindexstart"][ui]), int(m["ion_uniquelevelindexstart"][ui + 1])
    dropped = sorted(int(start[ul]) + t for ul in range(lo, hi) for t in range(int(nt[ul])))
    assert dropped and hm.ncovered == full.ncovered - len(dropped)
    assert (hm.conts[dropped] == -1).all()
    for ul in np.nonzero(nt > 0)[0]:
        for t in range(int(nt[ul])):
            row = int(start[ul]) + t
            assert full.conts[row].tolist() == [ul, t]
            assert hm.conts[row].tolist() == ([-1, -1] if row in dropped else [ul, t])
    got, whole = hm.tables(rc.TBMATH), full.tables(rc.TBMATH)
    covered = np.ones(hm.nbf, bool)
    covered[dropped] = False
    for k in rc.TABLES:
        assert got[k][~covered].tobytes() == bytes(8 * hm.tablesize * len(dropped))  # +0.0: all bits clear
        assert got[k][covered].tobytes() == whole[k][covered].tobytes() and (got[k][covered] > 0).all()
    assert not got["flags"].any()
    assert got["totals"]["integrals"] == 3 * hm.ncovered * hm.tablesize
    ul2 = int(np.nonzero(nt == 2)[0][0])
    r0 = int(start[ul2])
    assert full.conts[r0 + 1].tolist() == [ul2, 1] and not np.array_equal(whole["spontrecombcoeffs"][r0], whole["spontrecombcoeffs"][r0 + 1])


def test_node_count_and_threads(case):
    """every integral ends after its first node (nodes == integrals, none at depth 15), none is flagged, and the thread count does
    not enter"""
    hm = case["hm"]
    for out in (case["tb"], case["libm"]):
        t = out["totals"]
        assert t["integrals"] == hm.ntables * hm.ncovered * hm.tablesize and t["nodes"] == t["integrals"]
        assert t["at_depth_cap"] == 0 and t["flagged"] == 0 and not out["flags"].any()
    one = hm.tables(rc.TBMATH, shared=True, nthreads=1)
    rc.same_tables(one, case["tb"], case["preset"])
    assert one["totals"] == case["tb"]["totals"]


def test_two_table_build():
    """a build without USE_LUT_PHOTOION makes alpha_sp and bfcooling only"""
    hm = rc.HostModel(rc.model("nltenebular"), "nltenebular")
    out = hm.tables(rc.TBMATH)
    assert hm.ntables == 2 and out["corrphotoioncoeffs"] is None
    assert out["totals"]["integrals"] == out["totals"]["nodes"] == 2 * hm.ncovered * hm.tablesize
    assert (out["spontrecombcoeffs"] > 0).all() and (out["bfcooling_coeffs"] > 0).all()


def test_harness_under_the_sanitizers(tmp_path):
    """tests/ratecoeff_host/rows_main.cc, a program of its own built with -fsanitize=address,undefined: the threaded tables with both
    Math policies and in both forms, every table in an allocation of exactly its size; its counts are the library's"""
    case = _case("classic")
    subprocess.check_call(["make", "-C", rc.HOSTDIR, "rows_sanitized"], stdout=subprocess.DEVNULL)
    path = str(tmp_path / "call.bin")
    rc.dump_call(case["hm"], path)
    out = subprocess.run([os.path.join(rc.HOSTDIR, "rows_sanitized"), path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    t = case["tb"]["totals"]
    assert f"{4 * t['integrals']} integrals, {4 * t['nodes']} nodes, 0 flagged" in out.stdout, out.stdout
