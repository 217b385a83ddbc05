"""Shared by tests/test_initial_state_rules.py and tests/test_gpu_initial_state.py: the x86 build of artis_amd/csrc/initial_state.h
(tests/initial_state_host, made on first use, one library per options preset), its bodies applied to host arrays, a numpy restatement
of the same rules written from the reference (grid.cc:1077-1135, :1864-1926, decay.h:56-129, decay.cc:1052-1097), and the networks,
grids and set-ups both files use."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:  # run as a script (the networks for initial_state_host/rows_main.cc)
    sys.path.insert(0, os.path.dirname(HERE))

import decay_common as dc  # noqa: E402
import host_build  # noqa: E402
import packet_init_common as pc  # noqa: E402
from artis_amd import abi, synth  # noqa: E402

HOSTDIR = os.path.join(HERE, "initial_state_host")
DAY, T_MODEL, EPS = dc.DAY, dc.T_MODEL, dc.EPS
NETWORKS = ("small", "small_nohe4", "medium")
CLIGHT, STEBO, MH = 2.99792458e10, 5.670400e-5, 1.67352e-24
TANAKA_LIMITS = (0.1, 0.15, 0.20, 0.25, 0.30, 0.35)  # grid.cc:1884-1885
TANAKA_KAPPA = (19.5, 32.2, 22.3, 5.6, 5.36, 3.3)
_LIBS = {}


def lib(preset: str = "classic"):
    if preset in _LIBS:
        return _LIBS[preset]
    L = host_build.load(HOSTDIR, lambda p: f"libinitial_state_host_{p}.so", preset, only_this=True)
    L.init_host_last_error.restype = C.c_char_p
    L.init_host_mintemp.restype = L.init_host_maxtemp.restype = C.c_double
    L.init_host_decaychain_expansion.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    L.init_host_validate.restype = C.c_char_p
    L.init_host_validate.argtypes = [C.POINTER(abi.InitialParams), C.c_int64, C.c_double]
    L.init_host_new.restype = C.c_void_p
    L.init_host_new.argtypes = [C.POINTER(abi.DecayModel), C.POINTER(abi.DepositionModel), C.POINTER(abi.PacketInitModel), C.c_int64, C.c_double]
    L.init_host_free.argtypes = [C.c_void_p]
    L.init_host_energy.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 3
    L.init_host_cells.argtypes = [C.c_void_p, C.POINTER(abi.InitialParams), C.c_void_p, C.c_double] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 8 + [C.c_int]
    L.init_host_grey.argtypes = [C.c_void_p, C.POINTER(abi.InitialParams), C.c_double] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4
    _LIBS[preset] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def temperature_bounds(preset: str = "classic"):
    """(MINTEMP, MAXTEMP) of the preset's library"""
    L = lib(preset)
    return float(L.init_host_mintemp()), float(L.init_host_maxtemp())


def decaychain_expansion(lambdas, timediff: float):
    """(abundance, scale, x_dom) of the harness's Bateman sum with the expansion factor (the last decay constant counts as 0)"""
    lam = np.ascontiguousarray(lambdas, np.float64)
    out = np.zeros(3)
    lib().init_host_decaychain_expansion(_p(lam), len(lam), float(timediff), _p(out))
    return tuple(out)


def validate(params: dict, ncell: int, t_model: float) -> str:
    p, keep = abi.initial_params(params)
    return lib().init_host_validate(C.byref(p), ncell, t_model).decode()


class HostInitial:
    """the x86 build's bodies over a decay model, a deposition model and a pellet model (dicts over the structs' fields) of a grid"""

    def __init__(self, dm: dict, em: dict, pm: dict, model: abi.Model, preset: str = "classic"):
        self.L = lib(preset)
        self.n, self.np = int(model["npts_nonempty"]), len(dm["path_start"]) - 1
        self.rmax = float(model["rmax"])
        d, keep_d = abi.decay_model(dm)
        m, keep_m = abi.deposition_model(em)
        q, keep_q = abi.packet_init_model(pm)
        h = self.L.init_host_new(C.byref(d), C.byref(m), C.byref(q), self.n, float(model["tmin"]))
        assert h, self.L.init_host_last_error().decode()
        self.h = C.c_void_p(h)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.init_host_free(self.h)

    def energy(self, tstart: float) -> dict:
        out = dict(energy_vector=np.zeros(max(self.np, 1)), path_scale=np.zeros(max(self.np, 1)), path_x_dom=np.zeros(max(self.np, 1)))
        self.L.init_host_energy(self.h, float(tstart), _p(out["energy_vector"]), _p(out["path_scale"]), _p(out["path_x_dom"]))
        return {k: v[: self.np] for k, v in out.items()}

    def cells(self, params: dict, E, rho, massfrac, elem_anumber, nthreads: int = 8) -> dict:
        """every cell with the vector E and the decay update's rho [n] and elem_massfracs [n, nelements] at tstart"""
        p, keep = abi.initial_params(params)
        E = np.ascontiguousarray(E, np.float64)
        rho, mf, Z = np.ascontiguousarray(rho, np.float32), np.ascontiguousarray(massfrac, np.float32), np.ascontiguousarray(elem_anumber, np.int32)
        assert E.shape == (self.np,) and rho.shape == (self.n,) and mf.size == self.n * len(Z)
        out = abi.initial_arrays(self.n, 0)
        counts, first = np.zeros(5, np.int64), np.zeros(1, np.int32)
        self.L.init_host_cells(self.h, C.byref(p), _p(E), self.rmax, _p(rho), _p(mf), _p(Z), len(Z),
                               *[_p(out[k]) for k in ("T_initial", "endecay_per_mass", "kappagrey", "grey_depth", "thick", "flags")], _p(counts), _p(first), nthreads)
        out["ncells_branch"] = {k: int(counts[i]) for i, k in enumerate(abi.INITIAL_BRANCHES)}
        out["ncells_kappa_invalid"], out["first_nonfinite_cell"] = int(counts[4]), int(first[0])
        return out

    def grey(self, params: dict, rho, massfrac, elem_anumber, T_R) -> dict:
        """kappagrey, grey_depth and thick of every cell from temperatures given"""
        p, keep = abi.initial_params(params)
        rho, mf, Z = np.ascontiguousarray(rho, np.float32), np.ascontiguousarray(massfrac, np.float32), np.ascontiguousarray(elem_anumber, np.int32)
        T = np.ascontiguousarray(T_R, np.float32)
        out = dict(kappagrey=np.zeros(self.n, np.float32), grey_depth=np.zeros(self.n, np.float32), thick=np.zeros(self.n, np.int32))
        self.L.init_host_grey(self.h, C.byref(p), self.rmax, _p(rho), _p(mf), _p(Z), len(Z), _p(T), _p(out["kappagrey"]), _p(out["grey_depth"]), _p(out["thick"]))
        return out


# ---- the numpy restatement, written from the reference

def np_decaychain_expansion(lambdas, timediff: float):
    """calculate_decaychain(1., lambdas, timediff, true) decay.h:56-129 with the last decay constant zeroed (decay.cc:500-504) and the
    underflow clamp of the rule header; (abundance, scale, x_dom) with the scale of the summands before their cancellation"""
    lam = [float(x) for x in lambdas]
    lam[-1] = 0.0
    n = len(lam)
    lambdaproduct = 1.0
    for j in range(n - 1):
        lambdaproduct *= lam[j]
    total = maxabsterm = maxinv = x_dom = 0.0
    for j in range(n):
        denominator = 1.0
        for p in range(n):
            if p != j:
                denominator *= lam[p] - lam[j]
        term = 0.0
        x = lam[j] * timediff
        if x > 0.0:
            term = (math.exp(-x) + (math.expm1(-x) / x)) / denominator
            if 1.0 / abs(denominator) > maxinv:
                maxinv, x_dom = 1.0 / abs(denominator), x
        total += term
        maxabsterm = max(maxabsterm, abs(term))
    last = lambdaproduct * total
    abund = last
    if last < 0.0 or abs(total) <= n * EPS * maxabsterm or lambdaproduct * maxabsterm < 2.2250738585072014e-308:
        abund = 0.0
    return abund, lambdaproduct * maxinv, x_dom


def path_factor(dm: dict, em: dict, pm: dict, p: int) -> float:
    """branchproduct * lastdecayenergy / nucmass(top) of path p (decay.cc:1091-1093, :238-248), in the reference's order"""
    nuc = dm["path_nucindex"][dm["path_start"][p]: dm["path_start"][p + 1]]
    last = int(nuc[-2])
    endecay = float(em["nuc_endecay_gamma"][last]) + float(np.asarray(em["nuc_endecay_particle"]).reshape(-1, 6)[last, int(dm["path_last_decaytype"][p])])
    return endecay / float(pm["nuc_decay_daughters_probsum"][last]), float(dm["path_branchproduct"][p]), float(dm["nuc_a"][int(nuc[0])]) * MH


def np_energy(dm: dict, em: dict, pm: dict, tstart: float) -> dict:
    """calc_energy_per_massoftopnuc_decaypath_withexpansion decay.cc:1086-1097: energy_vector, path_scale, path_x_dom"""
    npaths = len(dm["path_start"]) - 1
    out = dict(energy_vector=np.zeros(npaths), path_scale=np.zeros(npaths), path_x_dom=np.zeros(npaths))
    for p in range(npaths):
        abund, scale, x = np_decaychain_expansion(dc.path_lambdas(dm, p), tstart - float(dm["t_model"]))
        lastdecayenergy, branch, mass = path_factor(dm, em, pm, p)
        out["energy_vector"][p] = branch * abund * lastdecayenergy / mass
        out["path_scale"][p], out["path_x_dom"][p] = scale, x
    return out


def energy_bound(dm: dict, em: dict, pm: dict, scale, x_dom) -> np.ndarray:
    """per path 4 (L + x_dom) 2^-52 scale * branchproduct * lastdecayenergy / nucmass(top): the cap of tests/test_decay_update_rules.py
    with the expansion sum's scale"""
    L = np.diff(dm["path_start"]).astype(np.float64)
    f = np.array([(lambda e, b, m: b * e / m)(*path_factor(dm, em, pm, p)) for p in range(len(L))])
    return 4.0 * (L + np.asarray(x_dom)) * EPS * np.asarray(scale) * f


def np_kappagrey(params: dict, c: int, rho_tmin, T_R, massfrac_c, elem_anumber) -> np.float32:
    """calculate_cell_kappagrey grid.cc:1864-1926"""
    if float(rho_tmin) <= 0.0:
        return np.float32(0.0)
    t = int(params["rpkt_grey_type"])
    if t == abi.GREY_FEGROUP_APPROX:
        kappa = ((0.9 * float(np.float32(params["ffegrp"][c]))) + 0.1) * 0.1 / ((0.9 * float(params["mfegroup"]) / float(params["mtot_input"])) + 0.1)
    elif t == abi.GREY_TANAKA2020:
        Ye = float(np.float32(params["initelectronfrac"][c]))
        kappa = next((k for lim, k in zip(TANAKA_LIMITS, TANAKA_KAPPA) if Ye <= lim), 0.96)
    else:
        X_lan = 0.0
        for z, x in zip(elem_anumber, massfrac_c):
            if 57 <= int(z) <= 71:
                X_lan += float(np.float32(x))
        if X_lan < 1e-7:
            kappa = 0.2
        elif X_lan < 1e-3:
            kappa = 3 * math.pow(X_lan / 1e-3, 0.3)
        elif X_lan < 1e-1:
            kappa = 3 * math.pow(X_lan / 1e-3, 0.5)
        else:
            kappa = 30 * math.pow(X_lan / 1e-1, 0.1)
        T_rad = float(np.float32(T_R))
        if T_rad < 2000.0:
            r = T_rad / 2000.0
            kappa *= ((r * r) * (r * r)) * r
    return np.float32(kappa)


def np_cells(params: dict, E, dm: dict, pm: dict, model: abi.Model, radial, rho, massfrac, elem_anumber, mintemp: float, maxtemp: float, vpkt_on: bool = False) -> dict:
    """assign_initial_temperatures grid.cc:1102-1134 per cell, then kappagrey and the first thickness (update_grid.cc:606-627)"""
    n, nn = int(model["npts_nonempty"]), len(dm["nuc_z"])
    X = np.asarray(dm["initnucmassfrac"], np.float32).reshape(n, nn)
    top = np.asarray(dm["path_nucindex"])[np.asarray(dm["path_start"])[:-1]]
    channel = bool(pm.get("initial_packets_on")) and bool(pm.get("use_model_initial_energy"))
    tmin, tstart, rmax = float(model["tmin"]), float(params["tstart"]), float(model["rmax"])
    out = abi.initial_arrays(n, 0)
    mf = np.asarray(massfrac, np.float32).reshape(n, -1)
    for c in range(n):
        terms = X[c, top].astype(np.float64) * np.asarray(E, np.float64)
        s = float(np.cumsum(terms)[-1]) if len(terms) else 0.0  # (np.cumsum adds in order)
        e = s + (float(pm["initenergyq"][c]) if channel else 0.0)
        rho_tmin = float(np.float32(dm["rho_tmin"][c]))
        with np.errstate(all="ignore"):  # (an overflowing product is the non-finite branch)
            r = np.float64(tmin / tstart)
            T = np.float32(np.power(np.float64(CLIGHT / 4 / STEBO) * (r * r * r) * np.float64(rho_tmin) * np.float64(e), 1.0 / 4.0))
        flag = abi.INITIAL_INSIDE
        if not np.isfinite(T):
            T, flag = np.float32(mintemp), abi.INITIAL_NONFINITE
        elif T < np.float32(mintemp):
            T, flag = np.float32(mintemp), abi.INITIAL_BELOW_MINTEMP
        elif T > np.float32(maxtemp):
            T, flag = np.float32(maxtemp), abi.INITIAL_ABOVE_MAXTEMP
        kappa = np_kappagrey(params, c, rho_tmin, T, mf[c], elem_anumber)
        tratmid = tstart / tmin
        dist = max((rmax * tratmid) - (float(radial[c]) * tratmid), 0.0)
        depth = np.float32(float(np.float32(kappa) * np.float32(rho[c])) * dist)  # (float x float first, update_grid.cc:611-612)
        if depth >= float(params["optical_depth_is_thick"]) and int(params["nts_first"]) < int(params["num_grey_timesteps"]):
            thick = abi.CELL_THICK
        elif vpkt_on and depth > float(params["optical_depth_is_thick_vpkt"]):
            thick = abi.CELL_THICK_VPKT_ONLY
        else:
            thick = abi.CELL_THIN
        out["T_initial"][c], out["endecay_per_mass"][c], out["kappagrey"][c], out["grey_depth"][c] = T, e, kappa, depth
        out["thick"][c], out["flags"][c] = thick, flag
    return out


# ---- the set-ups

GRIDS = {"1d": abi.GRID_SPHERICAL1D, "2d": abi.GRID_CYLINDRICAL2D, "3d": abi.GRID_CARTESIAN3D}
HUGE = 1.7e308  # a finite energy per mass whose product with CLIGHT / 4 / STEBO * rho_tmin overflows (the set-ups refuse an infinite one)
NONFINITE_CELL = 3


def calculated_meanweight(preset: str) -> bool:
    """the preset's build has USE_CALCULATED_MEANATOMICWEIGHT (kilonova_lte and what is built on it)"""
    return "kilonova" in preset


def first_timestep(model: abi.Model) -> abi.Timestep:
    """timestep 0 of a run that starts at the model's tmin with logarithmic steps of 5 per cent"""
    return synth.make_timestep(float(model["tmin"]), width_frac=0.05, vmax=float(model["vmax"]), nts=0)


@functools.lru_cache(maxsize=None)
def case(grid: str, kind: str, channel: bool, preset: str = "classic"):
    """(model, cs, dm, em, pm) as packet_init_common.case, for a grid built with the preset's options (classic builds: with
    elem_meannucmass, which their ion balance reads). kind "small20": the first 20 paths of the small network, fewer than the
    CKPT_DEPTH lines a lane of the cell walk keeps in flight."""
    gt = GRIDS[grid]
    if gt == abi.GRID_CYLINDRICAL2D:
        model, cs, ts, aux = synth.build("small", ncoord=6, gridtype=gt, options=preset)
    else:
        model, cs, ts, aux = dc.grid(gt, preset)
    if not calculated_meanweight(preset):
        model = synth.with_meannucmass(model)
    net = synth.decay_network("small" if kind == "small20" else kind)
    if kind == "small20":
        start = np.asarray(net["path_start"])[:21]
        net = dict(net, path_start=start, path_nucindex=np.asarray(net["path_nucindex"])[: start[-1]],
                   path_branchproduct=np.asarray(net["path_branchproduct"])[:20], path_last_decaytype=np.asarray(net["path_last_decaytype"])[:20])
    dm = synth.decay_model(model, cs, aux, net, t_model=T_MODEL)
    em = synth.deposition_model(model, net)
    pm = synth.packet_init_model(model, net, em, pc.TMAX, initial_energy=channel)
    zc = pc.ZERO_CELL % int(model["npts_nonempty"])
    dm["initnucmassfrac"] = np.array(dm["initnucmassfrac"], np.float32)
    dm["initnucmassfrac"][zc, :] = 0.0
    if channel:
        pm["initenergyq"][zc] = 0.0
    return model, cs, dm, em, pm


def tstart_of(model: abi.Model) -> float:
    """timesteps[0].mid of a run that starts at the model's tmin with logarithmic steps of 5 per cent"""
    return float(synth.make_timestep(float(model["tmin"]), width_frac=0.05, nts=0).c.mid)


def step_params(model: abi.Model, cs, rpkt_grey_type: int, depth_is_thick: float = 1e3) -> dict:
    """a dict over artis_initial_params for the first step (nts 0 of 2 grey steps) of a grid made by synth.build()"""
    p = synth.initial_model(model, cs, rpkt_grey_type)
    p.update(tstart=tstart_of(model), nts_first=0, num_grey_timesteps=2, optical_depth_is_thick=depth_is_thick, optical_depth_is_thick_vpkt=0.5 * depth_is_thick)
    return p


def four_branches(dm: dict, pm: dict, model: abi.Model, E, preset: str = "classic"):
    """Copies (dm, pm, E) whose cells take all four branches of grid.cc:1113-1128: rho_tmin of every fifth cell scaled so that T_initial
    falls to half of MINTEMP, of every seventh (from cell 2: cell 1 is packet_init_common's cell without energy) so that it rises to twice MAXTEMP, and one cell (NONFINITE_CELL) whose energy per mass
    is HUGE, so that the product under the root overflows: with the initial-energy channel its initenergyq; without it the vector's
    entry of path 0, whose top nuclide then only that cell holds (half of its mass). An infinite initenergyq, rho_tmin or vector entry
    is refused by the set-ups' validators, on the device as in the harness."""
    n, nn = int(model["npts_nonempty"]), len(dm["nuc_z"])
    mintemp, maxtemp = temperature_bounds(preset)
    channel = bool(pm.get("initial_packets_on")) and bool(pm.get("use_model_initial_energy"))
    top = np.asarray(dm["path_nucindex"])[np.asarray(dm["path_start"])[:-1]]
    dm2, pm2, E2 = dict(dm), dict(pm), np.array(E, np.float64)
    X = np.array(dm["initnucmassfrac"], np.float32).reshape(n, nn)
    bad = NONFINITE_CELL % n
    if channel:
        q = np.array(pm["initenergyq"], np.float64)
        q[bad] = HUGE
        pm2["initenergyq"] = q
    else:
        X[:, top[0]] = 0.0
        X[bad, top[0]] = 0.5
        E2[0] = HUGE
        dm2["initnucmassfrac"] = X
    e = X[:, top].astype(np.float64) @ np.where(E2 == HUGE, 0.0, E2) + (np.asarray(pm["initenergyq"]) if channel else 0.0)
    tmin, tstart = float(model["tmin"]), tstart_of(model)
    rho = np.asarray(dm["rho_tmin"], np.float64).copy()
    T = (CLIGHT / 4 / STEBO * (tmin / tstart) ** 3 * rho * e) ** 0.25
    ok = (e > 0) & (np.arange(n) != bad)
    low, high = ok & (np.arange(n) % 5 == 0), ok & (np.arange(n) % 7 == 2)
    rho[low] *= (0.5 * mintemp / T[low]) ** 4
    rho[high] *= (2.0 * maxtemp / T[high]) ** 4
    dm2["rho_tmin"] = rho.astype(np.float32)
    return dm2, pm2, E2


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for kind in NETWORKS:
        dc.dump_network(synth.decay_network(kind), [14, 26, 27], os.path.join(sys.argv[1], kind + ".txt"))
