"""The rules of artis_amd/csrc/photoion.h (get_corrphotoioncoeff without the table, ratecoeff.cc:463-521 and 840-868) on x86
(tests/photoion_host): the libm build against a Python restatement of the reference bit for bit, the stage's own exp / expm1 against
libm's, a smooth case against a fine-grid quadrature, the selection between estimator and integral, edge cells, determinism and the
harness under the sanitizers. Models: synth "small" on 3 cells per axis (19 non-empty cells x 159 continua) with the options of nltenebular and
ci_nebular_limitbfest (estimators for a subset of the continua)."""
import math
import os
import subprocess

import numpy as np
import pytest

import photoion_common as pc
from artis_amd import abi

# constants.h
H, KB, CLIGHT, SAHACONST, PI = 6.6260755e-27, 1.38064852e-16, 2.99792458e10, 2.0706659e-16, 3.14159265358979323846
HOVERKB = H / KB
FOURPI = 4 * PI
EPSREL = 1e-3


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
    """ratecoeff.cc:463-521, radfield.cc:786 with select_bin (radfield.cc:138, sn3d.h:115) and gausskronrod.h:173-257 in scalar Python
    floats (IEEE doubles; glibc's exp / expm1 / pow through math). Cross-sections: the interpolated form (atomic.h:202), which every
    build without USE_LUT_PHOTOION has."""

    def __init__(self, model, hm, ins):
        import ratecoeff_common as rc

        self.m, self.hm, self.ins = model, hm, ins
        self.NP, self.INC = int(model["NPHIXSPOINTS"]), float(model["NPHIXSNUINCREMENT"])
        self.last = 1.0 + (self.INC * (self.NP - 1))
        self.gx, self.gw, self.gwg = (a.tolist() for a in rc.gk61_tables("nltenebular"))
        self.nu_min, self.nu_max, self.nu_super = (float(v) for v in hm.bin_consts)
        self.delta_nu = (self.nu_max - self.nu_min) / (hm.nbins - 1)
        self.binned = bool(hm.multibin) and ins["nts"] >= hm.first_nlte
        n, nl, nb = hm.n, hm.nlevels, hm.nbins
        self.pops = np.asarray(ins["levelpops"], np.float64).reshape(n, nl)
        self.binW = np.asarray(ins["radfieldbin_W"], np.float32).reshape(n, nb)
        self.binT = np.asarray(ins["radfieldbin_T_R"], np.float32).reshape(n, nb)
        self.nodes = self.integrals = 0

    def sigma(self, xs, nu_edge, nu):
        NP, INC = self.NP, self.INC
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

    def select_bin(self, nu):  # radfield.cc:138
        if nu < self.nu_min:
            return -2
        if nu >= self.nu_super:
            return -1
        if nu >= self.nu_max:
            return self.hm.nbins - 1
        frac = (nu - self.nu_min) / self.delta_nu
        trunc = int(frac)
        b = trunc - 1 if frac < float(trunc) else trunc
        upper = self.nu_super if b == self.hm.nbins - 1 else self.nu_min + ((b + 1) * self.delta_nu)
        return b + 1 if nu == upper else b

    @staticmethod
    def planck(nu, T):
        return 2 * H * (nu * nu * nu) / (CLIGHT * CLIGHT) / c_expm1(HOVERKB * nu / T)

    def radfield(self, nu, c):  # radfield.cc:786
        if self.binned:
            b = self.select_bin(nu)
            if b >= 0:
                W = float(self.binW[c, b])
                if W >= 0.0:
                    return W * self.planck(nu, float(self.binT[c, b]))
            return 0.0
        return f32(self.ins["W"][c]) * self.planck(nu, f32(self.ins["TR"][c]))

    def consts(self, ul, t):
        m = self.m
        ui = int(np.searchsorted(np.asarray(m["ion_uniquelevelindexstart"]), ul, side="right")) - 1
        ts = int(m["level_phixstargetstart"][ul]) + t
        upper = int(m["ion_uniquelevelindexstart"][ui + 1]) + int(m["allphixstargets_levelindex"][ts])
        E_threshold = float(m["level_epsilon"][upper]) - float(m["level_epsilon"][ul])
        nu_threshold = (1.0 / H) * E_threshold  # a multiplication (ratecoeff.cc:485), unlike ratecoeff.cc:179
        start = int(m["level_phixsstart"][ul]) * self.NP
        return dict(upper=upper, g_lower=float(m["level_statweight"][ul]), g_upper=float(m["level_statweight"][upper]),
                    prob=float(m["allphixstargets_probability"][ts]), nu_threshold=nu_threshold, nu_max=nu_threshold * self.last,
                    xs=np.asarray(m["allphixs"])[start:start + self.NP])

    def ratio(self, ul, k, c):
        T_e = f32(self.ins["Te"][c])
        nnlevel, nnupper = float(self.pops[c, ul]), float(self.pops[c, k["upper"]])
        clumpednne = f32(np.float32(self.ins["nne"][c]) * np.float32(self.ins["clumpfactor"][c]))
        sahafact = SAHACONST * k["g_lower"] / k["g_upper"] * (math.pow(T_e, -1.5) if T_e == T_e else math.nan)
        r = nnupper / nnlevel * clumpednne * sahafact if nnlevel > 0.0 else 1.0
        return r if math.isfinite(r) else 0.0

    def integral(self, ul, t, c):  # calculate_corrphotoioncoeff_integral
        k = self.consts(ul, t)
        nu_edge, xs, T_e = k["nu_threshold"], k["xs"], f32(self.ins["Te"][c])
        ratio = self.ratio(ul, k, c)

        def f(x):
            corrfactor = 1.0 - (ratio * math.exp(-HOVERKB * x / T_e))
            if corrfactor < 0:
                corrfactor = 0.0
            return (1.0 / H) * self.sigma(xs, nu_edge, x + nu_edge) / (x + nu_edge) * self.radfield(x + nu_edge, c) * corrfactor

        self.integrals += 1
        return FOURPI * k["prob"] * self.adaptive(f, 0, k["nu_max"] - nu_edge, 15, 0.0)


_CASES = {}


def _case(preset):
    """the model of a preset, its cell state, the x86 build's view and the integrals of every entry in both Math policies (made once,
    never changed)"""
    if preset not in _CASES:
        model, cells, host_corr, aux = pc.state(preset)
        hm = pc.HostModel(model, preset)
        ins = pc.call_inputs(cells)
        _CASES[preset] = dict(preset=preset, model=model, cells=cells, hm=hm, ins=ins, libm=hm.compute(ins, pc.LIBM), tb=hm.compute(ins, pc.TBMATH))
    return _CASES[preset]


@pytest.fixture(scope="module", params=pc.PRESETS)
def case(request):
    return _case(request.param)


def _hex(a):
    return [float(v).hex() for v in np.asarray(a).ravel()]


def test_model_shape(case):
    hm = case["hm"]
    assert hm.n == 19 and hm.ncont == 159 and hm.nentries >= hm.ncont and hm.multibin and hm.detailed_bf and not hm.lut
    assert len(set(hm.conts[:, 2].tolist())) == hm.ncont  # one entry per continuum
    assert (hm.conts[:, 3] < 0).any() == (case["preset"] == "ci_nebular_limitbfest")


def test_libm_build_matches_the_reference_restated(case):
    """every entry of every cell, bit for bit; Tepow too; the restated walk's node count is the build's"""
    hm, got = case["hm"], case["libm"]
    ref = Restated(case["model"], hm, case["ins"])
    assert hm.tepow(case["cells"]["Te"]).tolist() == [math.pow(f32(T), -1.5) for T in case["cells"]["Te"]]
    for c in range(hm.n):
        for ul, t, entry, _ in hm.conts:
            want = ref.integral(int(ul), int(t), c)
            assert float(got["coeff"][c, entry]).hex() == want.hex(), (c, ul, t, got["coeff"][c, entry], want)
    assert got["totals"] == dict(from_estimators=0, integrals=ref.integrals, nodes=ref.nodes, at_depth_cap=0, nonfinite=0)
    print(f"{case['preset']}: {ref.integrals} integrals, {ref.nodes} nodes")
    written = np.zeros(hm.nentries, bool)
    written[hm.conts[:, 2]] = True
    assert (got["source"][:, written] == pc.SRC_INTEGRAL).all() and not got["source"][:, ~written].any()
    assert got["coeff"][:, ~written].tobytes() == bytes(8 * hm.n * int((~written).sum()))
    assert not got["flags"].any() and np.isfinite(got["coeff"]).all() and (got["coeff"][:, written] > 0).any()


# the largest relative difference between the TbMath and the libm build, measured on the two models of this file (the figures are
# printed below): 0 with the multibin field and with the dilute black body, where the exponential enters through 1 - ratio x exp with
# small ratios and tb_expm1 gives glibc's bits; 1.23e-15 in the edge cells (ratio 1: 1 - exp(-x) near the edge). The bar is four times
# the largest, the project's rule where no ulp table of the device's functions exists
MEASURED_TB_VS_LIBM = 1.23e-15


def _relative(a, b) -> float:
    big = np.abs(b) > 1e-280
    assert np.all(np.abs(a[~big] - b[~big]) <= 1e-280 * 2.2e-16)
    return float(np.max(np.abs(a[big] - b[big]) / np.abs(b[big]))) if big.any() else 0.0


def test_tbmath_against_libm(case):
    hm = case["hm"]
    early = pc.call_inputs(case["cells"], nts=pc.NTS_EARLY)
    edges = pc.call_inputs(pc.edge_cells(case["model"], case["cells"], hm))
    for label, tb, libm in (("multibin", case["tb"], case["libm"]), ("dilute black body", hm.compute(early, pc.TBMATH), hm.compute(early, pc.LIBM)),
                            ("edge cells", hm.compute(edges, pc.TBMATH), hm.compute(edges, pc.LIBM))):
        rel = _relative(tb["coeff"], libm["coeff"])
        print(f"{case['preset']} {label}: TbMath against libm, largest relative difference {rel:.3e}")
        assert rel <= 4 * MEASURED_TB_VS_LIBM, (label, rel)
        assert tb["source"].tobytes() == libm["source"].tobytes() and tb["flags"].tobytes() == libm["flags"].tobytes()
        assert tb["totals"] == libm["totals"]


def test_smooth_case_against_a_fine_grid_quadrature():
    """a flat cross-section table, the dilute black body (nts below FIRST_NLTE_RADFIELD_TIMESTEP) and ratio 0 (every upper population
    inf): the coefficient is 4 pi p sigma W (2 / c^2) int nu^2 / expm1(h nu / k T_R) dnu over [nu_edge, nu_max], taken here by
    Simpson's rule on 200001 points. Both policies within 1e-3, the integrator's requested epsrel."""
    model, cells, _, _ = pc.state("nltenebular")
    flat = abi.Model({**model.d, "allphixs": np.full(len(model["allphixs"]), 6e-18, np.float32)})
    hm = pc.HostModel(flat, "nltenebular")
    pops = np.array(cells["levelpops"], np.float64).reshape(hm.n, hm.nlevels)
    pops[:, np.unique(pc.upper_levels(flat, hm))] = np.inf
    ins = pc.call_inputs({**cells, "levelpops": pops.ravel()}, nts=pc.NTS_EARLY)
    ref = Restated(flat, hm, ins)
    sigma = f32(6e-18)
    worst = 0.0
    results = {m: hm.compute(ins, m) for m in (pc.LIBM, pc.TBMATH)}
    for c in (0, 9, 18):
        W, TR = f32(cells["W"][c]), f32(cells["TR"][c])
        for ul, t, entry, _ in hm.conts:
            k = ref.consts(int(ul), int(t))
            assert ref.ratio(int(ul), k, c) == 0.0
            nu = np.linspace(k["nu_threshold"], k["nu_max"], 200001)
            f = nu ** 2 / np.expm1(np.minimum(HOVERKB * nu / TR, 700.0))
            h = (k["nu_max"] - k["nu_threshold"]) / (len(nu) - 1)
            quad = h / 3 * (f[0] + f[-1] + 4 * f[1:-1:2].sum() + 2 * f[2:-1:2].sum())
            want = FOURPI * k["prob"] * sigma * W * (2 / (CLIGHT * CLIGHT)) * quad
            for m, out in results.items():
                rel = abs(out["coeff"][c, entry] - want) / want
                worst = max(worst, rel)
                assert rel <= 1e-3, (m, c, ul, t, rel)
    print(f"flat table, dilute black body: largest relative difference to the quadrature {worst:.2e}")


def test_selection(case):
    """estimators on: an entry whose continuum has an estimator >= 0 is (double)float exactly, source 1; a seeded negative one and a
    continuum without an estimator (limitbfest) are the integral, source 2; use_bf_estimators = 0: every entry is an integral"""
    hm, integrals = case["hm"], case["tb"]
    bf = pc.seeded_bfrate(hm.n, hm.nbfestim)
    out = hm.compute(pc.call_inputs(case["cells"], True, bf))
    nest = nint = 0
    for i, (ul, t, entry, bi) in enumerate(hm.conts):
        col = bf[:, bi] if bi >= 0 else np.full(hm.n, -1.0, np.float32)
        est = col >= 0
        assert (out["source"][est, entry] == pc.SRC_ESTIMATOR).all() and (out["source"][~est, entry] == pc.SRC_INTEGRAL).all()
        assert out["coeff"][est, entry].tobytes() == col[est].astype(np.float64).tobytes()
        assert out["coeff"][~est, entry].tobytes() == integrals["coeff"][~est, entry].tobytes()
        nest += int(est.sum())
        nint += int((~est).sum())
    assert nest > 0 and (bf < 0).any() and nint >= int((hm.conts[:, 3] < 0).sum()) * hm.n
    assert out["totals"]["from_estimators"] == nest and out["totals"]["integrals"] == nint and not out["flags"].any()
    assert (integrals["source"][:, hm.conts[:, 2]] == pc.SRC_INTEGRAL).all() and integrals["totals"]["from_estimators"] == 0
    assert integrals["totals"]["integrals"] == hm.n * hm.ncont
    # an estimator that is NaN is taken (NaN < 0 is false) and flagged
    bad = bf.copy()
    bi0 = int(hm.conts[hm.conts[:, 3] >= 0][0, 3])
    bad[4, bi0] = np.nan
    nan_out = hm.compute(pc.call_inputs(case["cells"], True, bad))
    assert nan_out["flags"].tolist() == [abi.PHOTOION_NONFINITE if c == 4 else 0 for c in range(hm.n)] and nan_out["totals"]["nonfinite"] == 1


def test_edge_cells(case):
    """one cell per edge (tests/photoion_common.py edge_cells); all finite and unflagged"""
    hm, model = case["hm"], case["model"]
    cells = pc.edge_cells(model, case["cells"], hm)
    ins = pc.call_inputs(cells)
    ref = Restated(model, hm, ins)
    entries = hm.conts[:, 2]
    for math_policy in (pc.TBMATH, pc.LIBM):
        out = hm.compute(ins, math_policy)
        base = case["tb" if math_policy == pc.TBMATH else "libm"]
        assert np.isfinite(out["coeff"]).all() and not out["flags"].any() and out["totals"]["nonfinite"] == 0
        assert out["coeff"][pc.EDGE_ALL_BINS_EMPTY].tobytes() == bytes(8 * hm.nentries)  # exactly +0
        assert out["coeff"][8:].tobytes() == base["coeff"][8:].tobytes()  # the cells that are no edge
        # ratio 1 with no lower population; the NaN population is not > 0 either: the same rule, the same bits
        for c in (pc.EDGE_NNLEVEL_ZERO, pc.EDGE_POP_NAN):
            assert all(ref.ratio(int(ul), ref.consts(int(ul), int(t)), c) == 1.0 for ul, t, _, _ in hm.conts)
        both = dict(cells, levelpops=np.where(np.isnan(cells["levelpops"]), 0.0, cells["levelpops"]))
        assert hm.compute(pc.call_inputs(both), math_policy)["coeff"][pc.EDGE_POP_NAN].tobytes() == out["coeff"][pc.EDGE_POP_NAN].tobytes()
        ratios = np.array([ref.ratio(int(ul), ref.consts(int(ul), int(t)), pc.EDGE_RATIO_HUGE) for ul, t, _, _ in hm.conts])
        assert (ratios > 1e20).all() and np.isfinite(ratios).all()
        assert all(ref.ratio(int(ul), ref.consts(int(ul), int(t)), pc.EDGE_UPPER_INF) == 0.0 for ul, t, _, _ in hm.conts)
        # a huge ratio clamps corrfactor to 0 where the exponential has not yet died: less than with ratio 0, never negative
        zero = dict(cells, levelpops=np.array(cells["levelpops"]).reshape(hm.n, hm.nlevels).copy())
        zero["levelpops"][pc.EDGE_RATIO_HUGE] = np.array(cells["levelpops"]).reshape(hm.n, hm.nlevels)[pc.EDGE_UPPER_INF]
        z = hm.compute(pc.call_inputs({**zero, "levelpops": zero["levelpops"].ravel()}), math_policy)["coeff"][pc.EDGE_RATIO_HUGE, entries]
        huge = out["coeff"][pc.EDGE_RATIO_HUGE, entries]
        assert (huge >= 0).all() and (huge <= z).all() and (huge < z).any()
        for c in (pc.EDGE_TE_MIN, pc.EDGE_TE_MAX):
            assert (out["coeff"][c, entries] >= 0).all() and out["coeff"][c, entries].any()
    # the libm build of the edge cells against the reference restated, bit for bit
    out = hm.compute(ins, pc.LIBM)
    for c in range(7):
        for ul, t, entry, _ in hm.conts[::5]:
            assert float(out["coeff"][c, entry]).hex() == ref.integral(int(ul), int(t), c).hex(), (c, ul, t)
    # the multibin field against the dilute black body
    early = hm.compute(pc.call_inputs(cells, nts=pc.NTS_EARLY))
    assert early["coeff"][9:].tobytes() != case["tb"]["coeff"][9:].tobytes() and (early["coeff"][pc.EDGE_ALL_BINS_EMPTY, entries] > 0).all()


def test_nonfinite_is_flagged_and_counted(case):
    """T_e = NaN in one cell: every coefficient of that cell is NaN, counted, and the cell alone is flagged"""
    hm = case["hm"]
    cells = pc.edge_cells(case["model"], case["cells"], hm, bad=True)
    for math_policy in (pc.TBMATH, pc.LIBM):
        out = hm.compute(pc.call_inputs(cells), math_policy)
        assert out["flags"].tolist() == [abi.PHOTOION_NONFINITE if c == pc.EDGE_TE_NAN else 0 for c in range(hm.n)]
        assert out["totals"]["nonfinite"] == hm.ncont and np.isnan(out["coeff"][pc.EDGE_TE_NAN, hm.conts[:, 2]]).all()
        assert np.isfinite(np.delete(out["coeff"], pc.EDGE_TE_NAN, axis=0)).all()


def test_determinism(case):
    hm = case["hm"]
    bf = pc.seeded_bfrate(hm.n, hm.nbfestim)
    ins = pc.call_inputs(case["cells"], True, bf)
    a, b, one = hm.compute(ins, nthreads=16), hm.compute(ins, nthreads=16), hm.compute(ins, nthreads=1)
    pc.same_result(a, b, "two calls")
    pc.same_result(a, one, "1 and 16 threads")


def test_harness_under_the_sanitizers(tmp_path):
    """tests/photoion_host/rows_main.cc, a program of its own built with -fsanitize=address,undefined: the threaded computation with both
    Math policies, every array in an allocation of exactly its size; its counts are the library's"""
    case = _case("nltenebular")
    hm = case["hm"]
    subprocess.check_call(["make", "-C", pc.HOSTDIR, "rows_sanitized"], stdout=subprocess.DEVNULL)
    bf = pc.seeded_bfrate(hm.n, hm.nbfestim)
    ins = pc.call_inputs(case["cells"], True, bf)
    path = str(tmp_path / "call.bin")
    pc.dump_call(hm, ins, path)
    out = subprocess.run([os.path.join(pc.HOSTDIR, "rows_sanitized"), path], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    t = hm.compute(ins)["totals"]
    assert f"{2 * t['from_estimators']} from estimators, {2 * t['integrals']} integrals, {2 * t['nodes']} nodes, 0 at the cap, 0 not finite, 0 cells flagged" in out.stdout, out.stdout
