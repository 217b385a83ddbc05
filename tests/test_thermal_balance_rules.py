"""The thermal-balance rules of artis_amd/csrc/thermal_balance.h -- the functions the engine's kernels call -- compiled for x86
(tests/thermal_host) and applied to synthetic inputs (tests/thermal_common.py synthetic_case): the cooling of every cell against the
oracle's cell cache; the renormalisation, Gamma per ground population, bound-free heating, deposition heating and adiabatic cooling
against a sequential restatement of the reference's lines (update_grid.cc:344-387, ratecoeff.cc:926-961, thermalbalance.cc:96-104,
:161-180); every branch of the finder on constructed cells; the condition the GPU test's T_e bar rests on (one sign change per
bracketed cell); the fixed order of combine64; and ARTIS_OPT_TEMPERATURE_SOLVER_ACCURACY of every preset against the reference's
options files (tests/golden/thermal_options_reference.json, recorded by tests/golden/make_thermal_options_golden.py)."""
import ctypes as C
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ionbal_common as ib
import thermal_common as tc
from artis_amd import abi, synth
from artis_amd.build import PRESETS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KB = 1.38064852e-16
f32, f64 = np.float32, np.float64
R = {k: i for i, k in enumerate(abi.THERMAL_RATES)}


@pytest.fixture(scope="module")
def case():
    return tc.synthetic_case()


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


class Restated:
    """the reference's loops over one model, sequential, in Python floats (glibc's exp / pow / log, as the x86 build)"""

    def __init__(self, model):
        d = model.d
        self.d = d
        self.eps = [float(x) for x in d["level_epsilon"]]
        self.g = [float(x) for x in np.asarray(d["level_statweight"], f32)]
        self.ion_uls = [int(x) for x in d["ion_uniquelevelindexstart"]]
        self.nion_lev = [int(x) for x in d["ion_nlevels_ionising"]]
        self.elem_nions = [int(x) for x in d["elem_nions"]]
        self.uiis = [int(x) for x in d["elem_uniqueionindexstart"]]
        self.lowest = [int(x) for x in d["elem_lowest_ionstage"]]
        self.ntargets = [int(x) for x in d["level_nphixstargets"]]
        self.targetstart = [int(x) for x in d["level_phixstargetstart"]]
        self.targetlevel = [int(x) for x in d["allphixstargets_levelindex"]]
        self.targetprob = [float(x) for x in d["allphixstargets_probability"]]
        self.bflist = [int(x) for x in d["level_bflist_start"]]
        self.closest = [int(x) for x in d["level_closestgroundlevelcont"]]
        self.phixsstart = [int(x) for x in d["level_phixsstart"]]
        self.npts = int(d["NPHIXSPOINTS"])
        self.allphixs = np.asarray(d["allphixs"], f32)
        self.ts, self.tmin_, self.tmax_ = synth.OPTION_TABLES["classic"]
        self.corr = np.asarray(d["corrphotoioncoeffs"], f64).reshape(-1, self.ts)
        self.tgrid = [float(x) for x in ib.HostModel(model).temperature_grid()]
        self.T_step_log = (math.log(self.tmax_) - math.log(self.tmin_)) / (self.ts - 1.0)
        self.minpop = ib.lib("classic").ib_host_minpop()
        self.ne = len(self.elem_nions)

    def upperindex(self, T):  # get_temperature_gridupperindex ratecoeff.cc:54
        gridsize = self.ts + 1
        index = min(max(int(math.log(T / self.tmin_) / self.T_step_log) + 1, 0), gridsize)
        while index > 0 and self.tgrid[index - 1] > T:
            index -= 1
        while index < gridsize and self.tgrid[index] <= T:
            index += 1
        return index

    def lerp(self, row, T):  # lerp_or_last ratecoeff.cc:524
        up = self.upperindex(T)
        if up == 0:
            return float(row[0])
        if up < self.ts:
            T_lower, T_upper = self.tgrid[up - 1], self.tgrid[up]
            f_lower, f_upper = float(row[up - 1]), float(row[up])
            return f_lower + ((f_upper - f_lower) / (T_upper - T_lower) * (T - T_lower))
        return float(row[self.ts - 1])

    def corrphotoion_ana(self, ul, t, T_R):
        return self.lerp(self.corr[self.bflist[ul] + t], float(T_R))

    def groundpop(self, stored, massfrac):  # get_groundlevelpop ltepop.h:75
        nn = float(stored)
        if nn < self.minpop:
            return self.minpop if massfrac > 0 else 0.0
        return nn

    def levelpop(self, ul, start, nnground, massfrac, T_exc):  # calculate_levelpop ltepop.cc:412
        if ul == start:
            nn = nnground
        else:
            nn = nnground * self.g[ul] / self.g[start] * _exp(-(self.eps[ul] - self.eps[start]) / KB / float(T_exc))
        if nn < self.minpop:
            nn = self.minpop if massfrac > 0 else 0.0
        return nn

    def col_ion(self, T_e, cnne, e, ion, ul, t, epsilon_trans):  # col_ionization_ratecoeff macroatom.cc:686
        stage = self.lowest[e] + ion
        g = 0.1 if stage == 1 else (0.2 if stage == 2 else 0.3)
        fac1 = epsilon_trans / KB / float(T_e)
        sigma_bf = float(self.allphixs[self.phixsstart[ul] * self.npts]) * self.targetprob[self.targetstart[ul] + t]
        return float(cnne) * 1.55e13 * math.pow(float(T_e), -0.5) * g * sigma_bf * _exp(-fac1) / fac1

    def iongamma_per_gspop(self, e, ion, gci, ground, massfrac, TJ, TR, W, Te, cnne, renorm):  # ratecoeff.cc:926-961
        if ion >= self.elem_nions[e] - 1 or gci[self.uiis[e] + ion] < 0:
            return 0.0
        ui = self.uiis[e] + ion
        start, ustart = self.ion_uls[ui], self.ion_uls[ui + 1]
        nnground = self.groundpop(ground[ui], massfrac[e])
        rad = coll = 0.0
        for level in range(self.nion_lev[ui]):
            ul = start + level
            nnlevel = self.levelpop(ul, start, nnground, massfrac[e], TJ)
            for t in range(self.ntargets[ul]):
                gammacorr = float(f64(W)) * self.corrphotoion_ana(ul, t, TR)
                if self.closest[ul] >= 0:
                    gammacorr *= float(renorm[self.closest[ul]])
                rad += nnlevel * gammacorr
                epsilon_trans = self.eps[ustart + self.targetlevel[self.targetstart[ul] + t]] - self.eps[ul]
                coll += nnlevel * self.col_ion(Te, cnne, e, ion, ul, t, epsilon_trans)
        rate = rad + coll
        return 0.0 if nnground <= 0 else rate / nnground


def _rel(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return np.max(np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300)), initial=0.0)


def test_cooling_of_resident_state_matches_oracle(case, oracle):
    """rates(Te = resident, rebalance = 0): cooling_ff + cooling_collisional + cooling_fb of every cell against the oracle's total of
    the cell's cooling list, to the bar of a reordered f64 sum (tests/test_gpu_parity.py: 1e-12)"""
    hm, ins, model = case["hm"], case["ins"], case["model"]
    resident = dict(ins, rho=case["state"]["rho"], massfrac=case["state"]["elem_massfracs"])  # rebalance = 0: the resident matter
    r = hm.rates(resident, Te=None, rebalance=False)["rates"]
    cs = abi.CellState(case["state"])
    worst = 0.0
    for c in range(hm.n):
        contribs = oracle.cellcache(model, cs, case["ts"], c)["ion_cooling_contribs"]
        total = float(contribs[-1])  # (cumulative over the ions, kpkt.cc:288-294)
        got = r[c, R["cooling_ff"]] + r[c, R["cooling_collisional"]] + r[c, R["cooling_fb"]]
        assert total > 0
        worst = max(worst, abs(got - total) / total)
    print(f"cooling against the oracle: worst relative difference {worst:.3e} over {hm.n} cells")
    assert worst <= 1e-12


def test_renormalisation_and_gamma_restated(case):
    hm, ins, s, model = case["hm"], case["ins"], case["solved"], case["model"]
    rs = Restated(model)
    gci = hm.gci()
    n, g = hm.n, hm.g
    gamma_normed = ib.gamma_normed(np.asarray(ins["gamma_raw"]).reshape(n, g), ins["assocvol"], ins["prev_mid"], ins["tmin"], ins["deltat"])
    res_renorm = np.asarray(ins["res_renorm"]).reshape(n, g)
    ion_of = {int(gi): ui for ui, gi in reversed(list(enumerate(gci))) if gi >= 0}
    ground = np.asarray(ins["res_ground"], f32).reshape(n, hm.ni)
    massfrac = np.asarray(ins["massfrac"], f32).reshape(n, hm.ne)
    worst = 0.0
    for c in range(n):
        exp_renorm = res_renorm[c].copy()
        if case["fitted"][c]:
            for gi, ui in ion_of.items():
                ana = float(f64(f32(ins["res_W"][c]))) * rs.corrphotoion_ana(rs.ion_uls[ui], 0, f32(ins["res_TR"][c]))
                ratio = gamma_normed[c, gi] / ana if ana > 0 else math.inf
                exp_renorm[gi] = ratio if math.isfinite(ratio) else 1.0
        assert np.array_equal(s["renorm"][c], exp_renorm), c  # arithmetic only: bit-equal
        if not case["fitted"][c]:
            assert not s["gamma"][c].any()
            continue
        cnne = f32(ins["clump"][c]) * f32(ins["res_nne"][c])
        for e in range(rs.ne):
            for ion in range(rs.elem_nions[e]):
                gi = gci[rs.uiis[e] + ion]
                if gi < 0:
                    continue
                want = rs.iongamma_per_gspop(e, ion, gci, ground[c], massfrac[c], f32(ins["res_TJ"][c]), f32(ins["res_TR"][c]),
                                             f32(ins["res_W"][c]), f32(ins["res_Te"][c]), cnne, exp_renorm)
                worst = max(worst, _rel(s["gamma"][c, gi], want))
    print(f"Gamma per ground population: worst relative difference {worst:.3e}")
    assert worst <= 1e-12
    assert (s["gamma"][case["fitted"]] > 0).any()


def test_heating_and_adiabatic_restated(case):
    hm, ins, s, model = case["hm"], case["ins"], case["solved"], case["model"]
    rs = Restated(model)
    n = hm.n
    massfrac = np.asarray(ins["massfrac"], f32).reshape(n, hm.ne)
    mw = np.asarray(model["elem_meannucmass"], f32)
    bfheat = np.asarray(ins["bfheat"], f64).reshape(n, hm.nl)
    worst = 0.0
    for c in np.nonzero(case["fitted"])[0]:
        r = s["rates"][c]
        lep, al, sf = float(ins["ntlepton_dep"][c]), float(ins["dep_alpha"][c]), float(ins["dep_spfission"][c])
        heating_dep = (lep * 1.0) + al + sf
        assert r[R["heating_dep"]] == heating_dep
        assert r[R["dep_frac_heating"]] == (heating_dep / (lep + al + sf) if (al + sf) > 0 else 1.0)
        # adiabatic cooling at the stored T_e (the float of the damped solution) with the final n_e: bit-equal
        T_e = float(f32(tc.damped(s["Te_solved"][c], ins["res_Te"][c], hm.mintemp, hm.maxtemp)))
        assert f32(T_e) == s["Te"][c]
        nntot = 0.0
        for e in range(rs.ne):
            nntot += float(f64(massfrac[c, e]) / f64(mw[e]) * f64(f32(ins["rho"][c])))
        nntot = nntot + float(s["nne"][c])
        vol, tmin, t = float(ins["assocvol"][c]), float(ins["tmin"]), float(ins["prev_mid"])
        p = nntot * KB * T_e
        dV_on_dt = 3 * vol / (tmin * tmin * tmin) * (t * t)
        V = vol * ((t / tmin) * (t / tmin) * (t / tmin))
        assert r[R["cooling_adiabatic"]] == p * dV_on_dt / V, c
        # bound-free heating with the final ground populations, sequential
        bf = 0.0
        for e in range(rs.ne):
            for ion in range(rs.elem_nions[e] - 1):
                ui = rs.uiis[e] + ion
                start = rs.ion_uls[ui]
                nnground = rs.groundpop(s["ground"][c, ui], massfrac[c, e])
                for level in range(rs.nion_lev[ui]):
                    bf += rs.levelpop(start + level, start, nnground, massfrac[c, e], f32(ins["fit_TJ"][c])) * bfheat[c, start + level]
        worst = max(worst, _rel(r[R["heating_bf"]], bf))
        total_h = r[R["heating_ff"]] + r[R["heating_bf"]] + r[R["heating_collisional"]] + r[R["heating_dep"]]
        total_c = r[R["cooling_ff"]] + r[R["cooling_fb"]] + r[R["cooling_collisional"]] + r[R["cooling_adiabatic"]]
        assert r[R["residual"]] == total_h - total_c
    print(f"bound-free heating: worst relative difference {worst:.3e}")
    assert worst <= 1e-12


def test_finder_bracketed_roots_hold_their_certificate(case):
    s = case["solved"]
    cells = np.nonzero((s["flags"] & abi.THERMAL_BRACKETED) != 0)[0]
    assert len(cells) > 0
    tc.certificate(case["hm"], case["ins"], s, s, cells)
    assert not (s["flags"] & abi.THERMAL_MAXIT).any()


def test_finder_branches_on_constructed_cells(case):
    hm, n = case["hm"], case["hm"].n
    fitted = np.nonzero(case["fitted"])[0]
    hot, cold, bad = (int(x) for x in fitted[:3])
    unfitted = int(np.nonzero(~case["fitted"])[0][0])
    ins = dict(case["ins"])
    for k in ("bfheat", "ntlepton_dep", "dep_alpha", "dep_spfission", "ff_raw", "col_raw"):
        ins[k] = np.array(ins[k], f64, copy=True)
    ins["ntlepton_dep"][hot] = 1e30  # heating everywhere
    for k in ("ntlepton_dep", "dep_alpha", "dep_spfission", "ff_raw", "col_raw"):  # no heating
        ins[k][cold] = 0.0
    ins["bfheat"] = ins["bfheat"].reshape(n, hm.nl)
    ins["bfheat"][cold] = 0.0
    ins["bfheat"][bad, 0] = np.inf  # (level 0 is an ionising ground level)
    s = hm.solve(ins)
    T_old = np.asarray(ins["res_Te"], f64)
    fl = s["flags"]
    assert fl[hot] & abi.THERMAL_PINNED_HIGH and not fl[hot] & (abi.THERMAL_BRACKETED | abi.THERMAL_PINNED_LOW | abi.THERMAL_NONFINITE)
    assert s["Te_solved"][hot] == hm.maxtemp and s["Te"][hot] == f32(min(2 * T_old[hot], hm.maxtemp)) and fl[hot] & abi.THERMAL_DAMPED_UP
    assert fl[cold] & abi.THERMAL_PINNED_LOW and not fl[cold] & (abi.THERMAL_BRACKETED | abi.THERMAL_PINNED_HIGH | abi.THERMAL_NONFINITE)
    assert s["Te_solved"][cold] == hm.mintemp and s["Te"][cold] == f32(max(0.5 * T_old[cold], hm.mintemp))
    assert fl[bad] & abi.THERMAL_NONFINITE and fl[bad] & abi.THERMAL_PINNED_LOW and s["Te_solved"][bad] == hm.mintemp
    for c in (hot, cold, bad):
        assert s["evals"][c] == 3 and np.array_equal(s["bracket"][c], [s["Te_solved"][c]] * 2)
    # the unfitted cell is untouched: the fit's T_e (T_J there), no flag, no evaluation, the resident populations
    assert s["Te"][unfitted] == f32(ins["fit_Te"][unfitted]) == f32(ins["fit_TJ"][unfitted])
    assert fl[unfitted] == 0 and s["evals"][unfitted] == 0 and not s["rates"][unfitted].any()
    assert np.array_equal(s["ground"][unfitted], np.asarray(ins["res_ground"], f32).reshape(n, hm.ni)[unfitted])
    # every other cell is as before
    same = np.ones(n, bool)
    same[[hot, cold, bad]] = False
    for k in ("Te", "Te_solved", "flags", "evals", "rates", "ground"):
        assert np.array_equal(s[k][same], case["solved"][k][same], equal_nan=True), k


def test_input_condition_of_the_gpu_bar(case):
    """asserted on the x86 rules' result: most fitted cells end bracketed and undamped, every other branch occurs, and the residual of
    every bracketed cell changes its sign exactly once over [MINTEMP, MAXTEMP] (64 log-spaced temperatures): the root two machines
    bracket is the same one"""
    hm, s, fitted = case["hm"], case["solved"], case["fitted"]
    fl = s["flags"]
    bracketed = (fl & abi.THERMAL_BRACKETED) != 0
    plain = bracketed & ((fl & (abi.THERMAL_DAMPED_UP | abi.THERMAL_DAMPED_DOWN)) == 0)
    assert 2 * plain.sum() >= fitted.sum(), (int(plain.sum()), int(fitted.sum()))
    for bit in (abi.THERMAL_PINNED_LOW, abi.THERMAL_PINNED_HIGH, abi.THERMAL_DAMPED_UP, abi.THERMAL_DAMPED_DOWN):
        assert ((fl & bit) != 0).any(), bit
    assert not (fl[~fitted]).any()
    T = np.geomspace(hm.mintemp, hm.maxtemp, 64)
    for c in np.nonzero(bracketed)[0]:
        r = hm.residuals(case["ins"], s, int(c), T)
        assert np.isfinite(r).all(), c
        assert np.count_nonzero(np.diff(np.sign(r))) == 1, (c, r)


def test_harness_under_the_sanitizers(case, tmp_path):
    """tests/thermal_host/rows_main.cc, a program of its own built with -fsanitize=address,undefined: the threaded solve, the rates with
    and without the ion balance and the residual scan on the 3D case and on a 1D one, every array in an allocation of exactly its size;
    its counts are the shared library's"""
    subprocess.check_call(["make", "-C", tc.HOSTDIR, "rows_sanitized"], stdout=subprocess.DEVNULL)
    cases = [case, tc.synthetic_case(abi.GRID_SPHERICAL1D)]
    paths = []
    for k, cs in enumerate(cases):
        paths.append(str(tmp_path / f"call{k}.bin"))
        tc.dump_call(cs["hm"], cs["ins"], paths[-1])
    out = subprocess.run([os.path.join(tc.HOSTDIR, "rows_sanitized")] + paths, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 2
    for cs, line in zip(cases, lines):
        s = cs["solved"]
        want = (f"{cs['hm'].n} cells, {int(cs['fitted'].sum())} fitted, {int(((s['flags'] & abi.THERMAL_BRACKETED) != 0).sum())} bracketed, "
                f"{int(s['evals'].sum())} evaluations")
        assert want in line, (want, line)


def test_copied_rate_coefficients_stay_in_step(case):
    """tb_col_exc and tb_col_ion, the stage's forms with its own exp and log, against physics.h's col_exc and col_ion over every upward
    transition and ionising target of the model: 8 ulp (1.8e-15 relative) -- two exp or one exp and one log within 2 ulp each, and the
    1 / sqrt for pow(T, -0.5)"""
    hm = case["hm"]
    hm.L.tb_host_ratecoeff_diff.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    worst = 0.0
    for T_e in (3500.0, 6000.0, 20000.0, 140000.0):
        out = np.zeros(3)
        hm.L.tb_host_ratecoeff_diff(hm.h, T_e, 1e8, out.ctypes.data_as(C.c_void_p))
        assert out[2] > 300
        worst = max(worst, out[0], out[1])
    print(f"copied rate coefficients: worst relative difference {worst:.3e}")
    assert worst <= 1.8e-15


def test_own_exp_and_log_against_libm():
    """tb_exp and tb_log, the plain-arithmetic exp and log the rates are formed with on both machines: within 2 ulp (4.5e-16 relative)
    of glibc's over the normal range -- fdlibm's forms stay below 1 ulp, glibc's own values below 1 ulp of the exact ones --, exact at
    the special arguments, and never further from glibc's than one spacing where the result is subnormal"""
    L = tc.lib()
    rng = np.random.default_rng(2)
    for x in np.concatenate([rng.uniform(-700, 709, 20000), rng.uniform(-1, 1, 10000), [0.5 * math.log(2), -0.5 * math.log(2), 709.78, -708.3]]):
        assert abs(L.tb_host_exp(float(x)) - math.exp(x)) <= 4.5e-16 * math.exp(x), x
    for x in np.concatenate([10.0 ** rng.uniform(-307, 308, 20000), rng.uniform(0.5, 2, 10000), [math.sqrt(2), math.sqrt(0.5), 5e-324, 1e-310]]):
        assert abs(L.tb_host_log(float(x)) - math.log(x)) <= 4.5e-16 * abs(math.log(x)), x
    assert L.tb_host_exp(0.0) == 1.0 and L.tb_host_log(1.0) == 0.0
    assert L.tb_host_exp(800.0) == math.inf and L.tb_host_exp(-800.0) == 0.0 and math.isnan(L.tb_host_exp(math.nan))
    assert L.tb_host_log(0.0) == -math.inf and math.isnan(L.tb_host_log(-1.0)) and L.tb_host_log(math.inf) == math.inf
    for x in rng.uniform(-745, -708.4, 2000):
        assert abs(L.tb_host_exp(float(x)) - math.exp(x)) <= 5e-324 + 4.5e-16 * math.exp(x), x


def test_combine64_order():
    rng = np.random.default_rng(1)
    p = rng.uniform(-1, 1, 64) * 10.0 ** rng.uniform(-8, 8, 64)
    q = p.copy()
    h = 32
    while h >= 1:
        q[:h] = q[:h] + q[h:2 * h]
        h //= 2
    assert tc.combine64(p) == q[0]


def test_temperature_solver_accuracy_pinned_to_the_reference():
    ref = json.load(open(os.path.join(HERE, "golden", "thermal_options_reference.json")))
    like = {"classic": "classic", "kilonova_lte": "kilonova_lte", "nltenebular": "nltenebular", "christinenonthermal": "christinenonthermal",
            "nltephotospheric": "nltephotospheric_dynamic_ion_range", "nltewithoutnonthermal": "nltewithoutnonthermal"}

    def reference_file(preset):
        if preset in like:
            return like[preset]
        if preset.startswith("kilonova") or preset.startswith("ci_kilonova"):
            return "kilonova_lte"
        if preset.startswith("classic") or preset.startswith("ci_classic"):
            return "classic"
        if preset.startswith("ci_nltephotospheric"):
            return "nltephotospheric_dynamic_ion_range"
        return "nltenebular"  # nltenebular_lineest, ci_nebular*

    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "p.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "artis_options.h"\nint main(void) { printf("%.17g\\n", (double)ARTIS_OPT_TEMPERATURE_SOLVER_ACCURACY); return 0; }\n')
        for preset in PRESETS:
            exe = os.path.join(tmp, preset)
            flags = [] if preset == "classic" else [f"-DARTIS_PRESET_{preset.upper()}"]
            subprocess.check_call(["gcc", *flags, "-I", os.path.join(ROOT, "include"), "-o", exe, src])
            got = float(subprocess.check_output([exe]))
            assert got == ref[reference_file(preset)]["TEMPERATURE_SOLVER_ACCURACY"], preset
    assert tc.lib("classic").tb_host_accuracy() == ref["classic"]["TEMPERATURE_SOLVER_ACCURACY"]
    assert tc.lib("classic").tb_host_supported() == 1 and tc.lib("kilonova_lte").tb_host_supported() == 0
