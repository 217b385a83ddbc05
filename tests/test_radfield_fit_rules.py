"""The radiation-field fit (artis_amd/csrc/radfield_fit.h) compiled for x86 (tests/radfield_host): its TOMS 748 against the
reference's solver (tests/golden/toms748_reference.json), its Planck integrals against mpmath quadrature, and its per-cell and
per-bin rules against a plain-Python restatement of update_grid_cell / set_params_fullspec / fit_parameters, bit for bit, on
hand-made edge cells."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import host_build
from artis_amd import abi, synth

HERE = os.path.dirname(os.path.abspath(__file__))
_HOSTDIR = os.path.join(HERE, "radfield_host")
_LIBS = {}
H, KB, PI, CLIGHT, STEBO = 6.6260755e-27, 1.38064852e-16, 3.14159265358979323846, 2.99792458e+10, 5.670400e-5
T_MIN, T_MAX = 500.0, 250000.0


def lib(preset="nltenebular"):
    if preset not in _LIBS:
        L = host_build.load(_HOSTDIR, lambda p: f"libradfield_host_{p}.so", preset)
        d, i, f = C.c_double, C.c_int, C.c_float
        for name, res, args in (("rf_host_partial", d, [d, i]), ("rf_host_planck_integral", d, [d, d, d, i]),
                                ("rf_host_mean_frequency", d, [d, d, d]), ("rf_host_mean_frequency_tail", d, [d, d, d]),
                                ("rf_host_mean_frequency_series", d, [d, d, d]), ("rf_host_mintemp", d, []), ("rf_host_maxtemp", d, []),
                                ("rf_host_nbins", i, []), ("rf_host_bin_edges", None, [C.c_void_p, C.c_void_p]),
                                ("rf_host_toms748_bin", i, [d, d, d, d, d, d, i, C.c_void_p]),
                                ("rf_host_toms748_analytic", i, [i, d, d, d, i, C.c_void_p]),
                                ("rf_host_find_bin_T_R", f, [d, d, d, C.POINTER(i), C.POINTER(i)]),
                                ("rf_host_fit_bin", i, [d, d, d, i, f, C.POINTER(f), C.POINTER(f)]),
                                ("rf_host_fit", None, [C.POINTER(abi.RadfieldConfig), d, C.c_int64, i, i, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.POINTER(abi.Radfield), i])):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIBS[preset] = L
    return _LIBS[preset]


def bin_edges(preset):
    L = lib(preset)
    n = 256 if L.rf_host_nbins() == 0 else L.rf_host_nbins()
    lo, hi = np.zeros(n), np.zeros(n)
    L.rf_host_bin_edges(lo.ctypes.data, hi.ctypes.data)
    return lo, hi


def host_fit(preset, model, cells: dict, est: abi.Estimators, prev_mid, deltat, vol, nprocs=1, lte=False, nbf=0, nline=0,
             bf_state=None, nthreads=1, ncell=None):
    """tests/radfield_host's rf_host_fit: the outputs of Engine.radfield_fit() from host arrays"""
    L = lib(preset)
    n = model["npts_nonempty"] if ncell is None else ncell
    nb = L.rf_host_nbins()
    cs = abi.CellState(cells)
    cfg, keep = abi.radfield_config(prev_mid, deltat, nprocs, vol, lte)
    out = abi.radfield_arrays(n, nb, nbf, nline)
    full = abi.radfield_arrays(n, 1, 1, 1)  # rf_host_fit writes every array it has
    for k in ("radfieldbin_T_R", "radfieldbin_W", "Jb_lu_normed", "Jb_lu_contribcount"):
        out.setdefault(k, full[k])
    if bf_state is None:
        bf_state = np.zeros(max(n * nbf, 1), np.float32)
    rf = abi.Radfield(struct_size=C.sizeof(abi.Radfield))
    abi.radfield_point(rf, out)
    L.rf_host_fit(C.byref(cfg), model["tmin"], n, nbf, nline, C.cast(cs.ref(), C.c_void_p), C.cast(est.ref(), C.c_void_p),
                  bf_state.ctypes.data, C.byref(rf), nthreads)
    if nb:
        out["radfieldbin_T_R"] = out["radfieldbin_T_R"].reshape(n, nb)
        out["radfieldbin_W"] = out["radfieldbin_W"].reshape(n, nb)
    if nbf:
        out["bfrate_normed"] = bf_state[: n * nbf].copy()
    out["totals"] = {k: int(rf.totals[i]) for i, k in enumerate(abi.RADFIELD_COUNTS)}
    return out


# ---- the plain-Python restatement (update_grid.cc:462-573, radfield.cc:253-441, :806-955) ----------------------------------
f32 = np.float32


def partial_py(x, times_nu):
    if x > 700:
        return 0.0
    s = 0.0
    for n in range(1, 1000):
        n2 = float(n * n)
        n3 = n2 * n
        n4 = n3 * n
        if times_nu:
            n5 = n4 * n
            x2 = x * x
            term = math.exp(-n * x) * (((x2 * x2) / n) + (4.0 * (x * x * x) / n2) + (12.0 * x2 / n3) + (24.0 * x / n4) + (24.0 / n5))
        else:
            term = math.exp(-n * x) * (((x * x * x) / n) + (3.0 * (x * x) / n2) + (6.0 * x / n3) + (6.0 / n4))
        s += term
        if term < s * 1e-15:
            break
    return s


def planck_integral_py(T, lo, hi):
    if T <= 0:
        return 0.0
    xl, xh = (H * lo) / (KB * T), (H * hi) / (KB * T)
    kb2, t2 = KB * KB, T * T
    factor = (2.0 * (kb2 * kb2) * (t2 * t2)) / ((H * H * H) * (CLIGHT * CLIGHT))
    return factor * (partial_py(xl, False) - partial_py(xh, False))


def clamp_py(T, lo_flag, hi_flag, flags, tmin, tmax):
    if T > tmax:
        return f32(tmax), flags | hi_flag
    if T < tmin:
        return f32(tmin), flags | lo_flag
    return T, flags


def fit_cell_py(J_raw, nuJ_raw, vol, prev_mid, tmin, deltat, nprocs, lte, thick, TJ, TR, Te, W, mintemp, maxtemp):
    q = prev_mid / tmin
    deltaV = vol * (q * q * q)
    enf = 1 / deltaV / deltat / nprocs
    nf = (1.0 / (4 * PI)) * enf
    J = J_raw * nf
    o = dict(J=J, nuJ=nuJ_raw, J_normfactor=nf, TJ=f32(TJ), TR=f32(TR), Te=f32(Te), W=f32(W), flags=0, enf=enf)
    if lte or thick == 1:
        try:
            T_J = f32(math.pow(J * PI / STEBO, 1.0 / 4.0))
        except ValueError:
            T_J = f32(np.nan)
        if not np.isfinite(T_J):
            T_J, o["flags"] = f32(TJ), o["flags"] | abi.RADFIELD_TJ_KEPT
        else:
            T_J, o["flags"] = clamp_py(T_J, abi.RADFIELD_TJ_LOW, abi.RADFIELD_TJ_HIGH, o["flags"], mintemp, maxtemp)
        o.update(TJ=T_J, TR=T_J, Te=T_J, W=f32(1.0))
        return o
    o["flags"] |= abi.RADFIELD_FITTED
    o["nuJ"] = nuJ_raw * nf
    with np.errstate(all="ignore"):
        nubar = float(np.float64(o["nuJ"]) / np.float64(J))
    if not math.isfinite(nubar) or nubar == 0.0:
        o["flags"] |= abi.RADFIELD_NUBAR_KEPT
        return o
    o["TJ"], o["flags"] = clamp_py(f32(math.pow(J * PI / STEBO, 1 / 4.0)), abi.RADFIELD_TJ_LOW, abi.RADFIELD_TJ_HIGH, o["flags"], mintemp, maxtemp)
    o["TR"], o["flags"] = clamp_py(f32(H * nubar / KB / 3.832229494), abi.RADFIELD_TR_LOW, abi.RADFIELD_TR_HIGH, o["flags"], mintemp, maxtemp)
    p2 = o["TR"] * o["TR"]  # float32 products: pow4 of a float
    o["W"] = f32(J * PI / STEBO / float(p2 * p2))
    return o


def fit_bin_py(L, J_raw, nuJ_raw, nf, b, Te, lo, hi, nbins):
    """fit_parameters for one bin; T_R of a solved bin from the x86 find_bin_T_R (the solver is checked against the golden data)"""
    J_bin = J_raw * nf
    bits = 0
    if not J_bin > 0:
        return f32(0.0), f32(0.0), 0
    if b == nbins - 1:
        T_R = f32(Te)
    else:
        fb, ev = C.c_int(0), C.c_int(0)
        T_R = f32(L.rf_host_find_bin_T_R(lo, hi, (nuJ_raw * nf) / J_bin, C.byref(fb), C.byref(ev)))
        bits |= fb.value
        bits |= 1 if T_R <= T_MIN else (2 if T_R >= T_MAX else 0)
    with np.errstate(all="ignore"):
        W = f32(np.float64(J_bin) / np.float64(planck_integral_py(float(T_R), lo, hi)))
        if W > 1e4 or not np.isfinite(W):
            bits |= 4
            W = f32(np.float64(J_bin) / np.float64(planck_integral_py(T_MAX, lo, hi)))
            if W > 1e4:
                return f32(-99.0), f32(0.0), bits | 8
            T_R = f32(T_MAX)
    return T_R, W, bits


# ---- tests ---------------------------------------------------------------------------------------------------------------------
def test_toms748_reproduces_reference_golden():
    with open(os.path.join(HERE, "golden", "toms748_reference.json")) as f:
        cases = json.load(f)["cases"]
    L = lib("nltenebular")
    out = np.zeros(2)
    nbin = 0
    for c in cases:
        fx = float.fromhex
        if c["kind"] == "bin":
            ev = L.rf_host_toms748_bin(fx(c["nu_lower"]), fx(c["nu_upper"]), fx(c["nu_bar"]), fx(c["ax"]), fx(c["bx"]), fx(c["tol"]),
                                       c["maxit"], out.ctypes.data)
            nbin += 1
        else:
            ev = L.rf_host_toms748_analytic(c["which"], fx(c["ax"]), fx(c["bx"]), fx(c["tol"]), c["maxit"], out.ctypes.data)
        assert (out[0].hex(), out[1].hex(), ev) == (c["lo"], c["hi"], c["evaluations"]), c
    assert nbin > 400 and len(cases) > nbin


def test_toms748_never_throws_on_bad_brackets():
    L = lib("nltenebular")
    out = np.zeros(2)
    assert L.rf_host_toms748_analytic(0, 1.0, 0.0, 1e-8, 100, out.ctypes.data) == 0 and np.isnan(out).all()  # a >= b
    assert L.rf_host_toms748_analytic(2, 1.0, 2.0, 1e-8, 100, out.ctypes.data) == 0 and np.isnan(out).all()  # no sign change


def test_planck_series_match_mpmath():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    L = lib("nltenebular")
    for x in np.geomspace(1e-3, 700.0, 29):
        for times_nu, p in ((0, 3), (1, 4)):
            # t = x + u, with exp(-x) taken out (quad's tolerance is absolute)
            xm = mpmath.mpf(float(x))
            ref = mpmath.exp(-xm) * mpmath.quad(lambda u: (xm + u) ** p * mpmath.exp(-u) / -mpmath.expm1(-(xm + u)),
                                                [0, 1, 4, 16, 64, mpmath.inf])
            got = L.rf_host_partial(float(x), times_nu)
            # the reference's series stops at 999 terms: below x ~ 0.03 that cuts off a tail of about sum_{n >= 1000} 6 / n^4
            # (x^3 integrand) relative to 6 zeta(4) ~ 3e-10; above it the epsrel = 1e-15 criterion ends the sum
            tol = 1e-12 if x >= 0.03 else 5e-10
            assert abs(got / float(ref) - 1) <= tol, (x, times_nu, got, ref)
    # mean frequency of bins of every kind (nltenebular bins and wide ones), both branches (x_low below and above 100)
    lo, hi = bin_edges("nltenebular")
    for T in (600.0, 3000.0, 1.5e4, 2.4e5):
        for b in (0, 40, 128, 254):
            xl, xh = H * lo[b] / (KB * T), H * hi[b] / (KB * T)
            if xl > 690:
                continue
            xm = mpmath.mpf(float(xl))
            num = mpmath.quad(lambda u: (xm + u) ** 4 * mpmath.exp(-u) / -mpmath.expm1(-(xm + u)), [0, xh - xl])
            den = mpmath.quad(lambda u: (xm + u) ** 3 * mpmath.exp(-u) / -mpmath.expm1(-(xm + u)), [0, xh - xl])
            ref = float(num / den) * KB * T / H
            got = L.rf_host_mean_frequency(T, lo[b], hi[b])
            # below x_low = 100 a bin's moment is the difference of two series from x to infinity (the reference's
            # calculate_planck_integral): a narrow bin at small x loses the digits the two have in common
            cancel = max(1.0, L.rf_host_partial(xl, 0) / (L.rf_host_partial(xl, 0) - L.rf_host_partial(xh, 0))) if xl < 100 else 1.0
            # (and below x ~ 0.03 the 999-term cut-off of each series, as above)
            assert abs(got / ref - 1) <= (1e-12 if xl >= 0.03 else 5e-10) * cancel, (T, b, xl, got, ref, cancel)
    # the two branches meet at x_low = 100
    for xl in (98.0, 99.5, 100.0, 100.5, 102.0):
        for width in (0.01, 0.5, 3.0):
            T = 1e4
            nl, nh = xl * KB * T / H, (xl + width) * KB * T / H
            a, b = L.rf_host_mean_frequency_tail(T, nl, nh), L.rf_host_mean_frequency_series(T, nl, nh)
            assert abs(a / b - 1) <= 1e-12, (xl, width, a, b)
    # Stefan-Boltzmann (integral over [0, inf) = 2 pi^4 k^4 T^4 / (15 h^3 c^2), which the constants' STEBO matches to 1e-5) and the
    # mean frequency 24 zeta(5) / (6 zeta(4)) kT/h = 3.832 kT/h (the 999-term series at x = 0 is short of the sum by ~3e-10)
    for T in (500.0, 1e4, 2.5e5):
        B = L.rf_host_planck_integral(T, 0.0, 1e30, 0)
        assert abs(B / (2 * PI ** 4 * KB ** 4 * T ** 4 / (15 * H ** 3 * CLIGHT ** 2)) - 1) < 1e-8
        assert abs(B / (STEBO * T ** 4 / PI) - 1) < 1e-5
        nubar = L.rf_host_planck_integral(T, 0.0, 1e30, 1) / B
        assert abs(nubar / (3.832229494 * KB * T / H) - 1) < 1e-8


@pytest.fixture(scope="module")
def nebular():
    model, cs, ts, aux = synth.build("small", ncoord=6, options="nltenebular")
    return model, cs, aux


def _edge_cells(mintemp, maxtemp, n):
    """(J_raw, nuJ_raw, thick, lte-cell?) rows at deltaV * deltat = 1e0 scale; the normalisation factor is applied by the rule"""
    sig = STEBO / PI
    rows = [
        (0.0, 0.0, 0), (1.0, 0.0, 0), (np.nan, 1.0, 0), (1.0, np.nan, 0),  # J = 0, nuJ = 0, NaN
        (sig * (3 * maxtemp) ** 4, sig * (3 * maxtemp) ** 4 * 3.832229494 * KB * 3 * maxtemp / H, 0),  # above MAXTEMP
        (sig * (0.2 * mintemp) ** 4, sig * (0.2 * mintemp) ** 4 * 3.832229494 * KB * 0.2 * mintemp / H, 0),  # below MINTEMP
        (sig * 6000.0 ** 4, sig * 6000.0 ** 4 * 3.832229494 * KB * 8000.0 / H, 0),  # plain
        (sig * 6000.0 ** 4, sig * 6000.0 ** 4 * 3.8 * KB * 8000.0 / H, 1),  # THICK
        (sig * (3 * maxtemp) ** 4, 1.0, 1), (sig * (0.2 * mintemp) ** 4, 1.0, 1), (np.nan, 1.0, 1), (0.0, 0.0, 1),
    ]
    return rows[:n]


def test_cells_match_python_restatement():
    """normalisation, T_J, the full-spectrum fit, W and the flags: x86 build == Python, bit for bit (classic: no bins)"""
    model, cs, ts, aux = synth.build("small", ncoord=6)
    L = lib("classic")
    mintemp, maxtemp = L.rf_host_mintemp(), L.rf_host_maxtemp()
    n = model["npts_nonempty"]
    vol = synth.assocvolume_tmin(model)
    prev_mid, deltat = 1.3 * model["tmin"], 0.05 * model["tmin"]
    for nprocs in (1, 2):
        for lte in (False, True):
            rows = _edge_cells(mintemp, maxtemp, 12)
            d = dict(cs.d)
            est = abi.Estimators(n, model["nbfcontinua_ground"])
            rng = np.random.default_rng(nprocs + 2 * lte)
            thick = np.zeros(n, np.int32)
            enf = 1 / (vol * (prev_mid / model["tmin"]) ** 3) / deltat / nprocs * (1.0 / (4 * PI))
            for c in range(n):
                if c < len(rows):
                    Jn, nuJn, thick[c] = rows[c]
                else:
                    T = rng.uniform(0.5 * mintemp, 1.5 * maxtemp)
                    Jn = STEBO / PI * T ** 4 * rng.uniform(0.01, 1.0)
                    nuJn = Jn * 3.832229494 * KB * T * rng.uniform(0.7, 1.3) / H
                    thick[c] = int(rng.random() < 0.2)
                est.J[c], est.nuJ[c] = Jn / enf[c], nuJn / enf[c]  # raw estimators that normalise to the row's J, nuJ
            d["thick"] = thick
            d["TJ"] = np.asarray(d["TJ"], np.float32) * 1.01
            h = host_fit("classic", model, d, est, prev_mid, deltat, vol, nprocs=nprocs, lte=lte)
            flags_seen = 0
            for c in range(n):
                p = fit_cell_py(est.J[c], est.nuJ[c], vol[c], prev_mid, model["tmin"], deltat, nprocs, lte, thick[c], d["TJ"][c],
                                np.float32(d["TR"][c]), np.float32(d["Te"][c]), np.float32(d["W"][c]), mintemp, maxtemp)
                for k in ("J", "nuJ", "J_normfactor"):
                    assert np.array_equal(np.float64(p[k]), h[k][c], equal_nan=True), (c, k, p[k], h[k][c])
                for k in ("TJ", "TR", "Te", "W"):
                    assert np.array_equal(f32(p[k]), h[k][c], equal_nan=True), (c, k, p[k], h[k][c], nprocs, lte)
                assert p["flags"] == h["flags"][c], (c, p["flags"], h["flags"][c])
                flags_seen |= p["flags"]
            want = abi.RADFIELD_TJ_LOW | abi.RADFIELD_TJ_HIGH | abi.RADFIELD_TJ_KEPT
            if not lte:
                want |= abi.RADFIELD_FITTED | abi.RADFIELD_NUBAR_KEPT | abi.RADFIELD_TR_LOW | abi.RADFIELD_TR_HIGH
            assert flags_seen & want == want, (flags_seen, want)


def test_bins_match_python_restatement(nebular):
    """fit_parameters per bin: J_bin = 0, the T_e superbin, the W retry and the -99 sentinel, no sign change at either end"""
    model, cs, aux = nebular
    L = lib("nltenebular")
    lo, hi = bin_edges("nltenebular")
    nb = L.rf_host_nbins()
    nf = 1e-3
    T = 8000.0
    cases = []
    for b in (3, 60, 200):
        B = planck_integral_py(T, lo[b], hi[b])
        nubar = L.rf_host_mean_frequency(T, lo[b], hi[b])
        cases += [(0.0, 0.0, b), (0.3 * B / nf, 0.3 * B * nubar / nf, b),  # J_bin = 0, a plain bin
                  (3e4 * B / nf, 3e4 * B * nubar / nf, b),  # W > 1e4 at T_R: retried at T_R_max
                  (1e40 * B / nf, 1e40 * B * nubar / nf, b),  # still > 1e4: -99
                  (B / nf, B * lo[b] * 0.999 / nf, b),  # nu_bar below the bin: the root lies below 500 K
                  (B / nf, B * hi[b] * 1.001 / nf, b)]  # above: beyond 250000 K
    cases += [(2e-9 / nf, 3e6 / nf, nb - 1), (0.0, 0.0, nb - 1)]  # the superbin takes T_e
    bits_seen = 0
    for J_raw, nuJ_raw, b in cases:
        tr, w = C.c_float(), C.c_float()
        hb = L.rf_host_fit_bin(J_raw, nuJ_raw, nf, b, C.c_float(7321.5), C.byref(tr), C.byref(w))
        pT, pW, pb = fit_bin_py(L, J_raw, nuJ_raw, nf, b, 7321.5, lo[b], hi[b], nb)
        assert (f32(tr.value), f32(w.value), hb) == (pT, pW, pb), (J_raw, nuJ_raw, b, tr.value, w.value, hb, pT, pW, pb)
        bits_seen |= hb
    assert bits_seen & 15 == 15, bits_seen


def test_bins_and_bf_of_a_population(nebular):
    """a whole nebular model through rf_host_fit: every fitted, unclamped bin brackets its nu_bar within the solver tolerance and
    has W * integral(B) = J_bin to float rounding; bound-free estimators normalised where not THICK, seeded values kept in THICK
    cells, nothing written with lte_iteration; the line estimators of the lineest build"""
    model, cs, aux = nebular
    L = lib("nltenebular")
    lo, hi = bin_edges("nltenebular")
    n, nb, nbf = model["npts_nonempty"], L.rf_host_nbins(), model["nbfcontinua"]
    vol = synth.assocvolume_tmin(model)
    prev_mid, deltat = 1.2 * model["tmin"], 0.1 * model["tmin"]
    rng = np.random.default_rng(5)
    est = abi.Estimators(n, model["nbfcontinua_ground"], nbfcontinua=nbf, nbins=nb)
    d = dict(cs.d)
    thick = (rng.random(n) < 0.15).astype(np.int32)
    d["thick"] = thick
    enf = 1 / (vol * (prev_mid / model["tmin"]) ** 3) / deltat * (1.0 / (4 * PI))
    for c in range(n):
        T = rng.uniform(3000.0, 30000.0)
        Wd = rng.uniform(1e-3, 0.5)
        for b in range(nb):
            Tb = T * rng.uniform(0.5, 2.0)
            B = Wd * planck_integral_py(Tb, lo[b], hi[b])
            est.radfieldbin_J[c * nb + b] = B / enf[c] * (rng.random() > 0.03)
            est.radfieldbin_nuJ[c * nb + b] = B * L.rf_host_mean_frequency(Tb, lo[b], hi[b]) / enf[c]
        est.J[c] = STEBO / PI * T ** 4 * Wd / enf[c]
        est.nuJ[c] = est.J[c] * 3.832229494 * KB * T / H
    est.bfrate_raw[:] = rng.uniform(0.0, 1e-20, n * nbf)
    seed = rng.uniform(1.0, 2.0, n * nbf).astype(np.float32)
    h = host_fit("nltenebular", model, d, est, prev_mid, deltat, vol, nbf=nbf, bf_state=seed.copy(), nthreads=4)
    fitted = (h["flags"] & abi.RADFIELD_FITTED) != 0
    assert fitted.sum() == (thick == 0).sum() > 20
    nchecked = 0
    for c in np.nonzero(fitted)[0]:
        for b in range(nb - 1):
            J_bin = est.radfieldbin_J[c * nb + b] * h["J_normfactor"][c]
            T_R, W = float(h["radfieldbin_T_R"][c, b]), float(h["radfieldbin_W"][c, b])
            if J_bin == 0:
                assert T_R == 0 and W == 0
                continue
            if not (T_MIN < T_R < T_MAX):
                continue
            nubar = est.radfieldbin_nuJ[c * nb + b] * h["J_normfactor"][c] / J_bin
            # (in a narrow bin at high T_R the mean frequency hardly moves with T_R: the residual's own rounding, ~1e-10 of nu_bar
            # after the series' cancellation, decides the root there)
            xl, xh = H * lo[b] / (KB * T_R), H * hi[b] / (KB * T_R)
            cancel = L.rf_host_partial(xl, 0) / (L.rf_host_partial(xl, 0) - L.rf_host_partial(xh, 0)) if xl < 100 else 1.0
            slack = (1e-13 if xl >= 0.03 else 1e-9) * cancel * nubar
            assert (L.rf_host_mean_frequency(T_R * (1 - 1.01e-4), lo[b], hi[b]) - slack <= nubar
                    <= L.rf_host_mean_frequency(T_R * (1 + 1.01e-4), lo[b], hi[b]) + slack), (c, b, T_R, nubar)
            assert abs(W * L.rf_host_planck_integral(T_R, lo[b], hi[b], 0) / J_bin - 1) <= 1.2e-7
            nchecked += 1
    assert nchecked > 1000
    # the bins of THICK cells keep the cell state's; counts add up
    assert np.array_equal(h["radfieldbin_T_R"][~fitted], np.asarray(d["radfieldbin_T_R"], np.float32).reshape(n, nb)[~fitted])
    assert h["totals"] == {k: int(h["cell_counts"][:, i].sum()) for i, k in enumerate(abi.RADFIELD_COUNTS)}
    # bound-free estimators (radfield.cc:920) and the seed in THICK cells
    bf = h["bfrate_normed"].reshape(n, nbf)
    enf_bf = 1 / (vol * (prev_mid / model["tmin"]) ** 3) / deltat / 1
    want = (est.bfrate_raw.reshape(n, nbf) * (enf_bf / H)[:, None]).astype(np.float32)
    assert np.array_equal(bf[thick == 0], want[thick == 0])
    assert np.array_equal(bf[thick == 1], seed.reshape(n, nbf)[thick == 1])
    h_lte = host_fit("nltenebular", model, d, est, prev_mid, deltat, vol, nbf=nbf, lte=True, bf_state=seed.copy())
    assert np.array_equal(h_lte["bfrate_normed"], seed) and not (h_lte["flags"] & abi.RADFIELD_FITTED).any()
