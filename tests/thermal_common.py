"""Shared by tests/test_thermal_balance_rules.py and tests/test_gpu_thermal_balance.py: the x86 build of artis_amd/csrc/thermal_balance.h
(tests/thermal_host, made on first use), its solve and rates applied to host arrays, and the synthetic inputs of the tests."""
import ctypes as C
import os

import numpy as np

import host_build
from artis_amd import abi, synth

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTDIR = os.path.join(HERE, "thermal_host")
H = 6.6260755e-27
KB = 1.38064852e-16
CELL_THICK = 1  # ARTIS_CELL_THICK
_LIBS = {}

# the order of the pointers a call hands over (thermal_host.cc enum Ptr)
INPUTS = ("res_TJ", "res_TR", "res_W", "res_Te", "res_nne", "res_ground", "res_U", "res_renorm", "fit_TJ", "fit_flags", "fit_Te", "rho",
          "massfrac", "meanweight", "clump", "gamma_raw", "ff_raw", "col_raw", "assocvol", "bfheat", "ntlepton_dep", "dep_alpha", "dep_spfission")
OUTPUTS = ("renorm", "gamma", "U", "Te", "nne", "Te_solved", "bracket", "evals", "flags", "rates", "ground", "phi")
_DTYPES = dict(fit_flags=np.int32, res_renorm=np.float64, gamma_raw=np.float64, ff_raw=np.float64, col_raw=np.float64, assocvol=np.float64,
               bfheat=np.float64, ntlepton_dep=np.float64, dep_alpha=np.float64, dep_spfission=np.float64)


def lib(preset: str = "classic"):
    if preset in _LIBS:
        return _LIBS[preset]
    L = host_build.load(HOSTDIR, lambda p: f"libthermal_host_{p}.so", preset)
    L.tb_host_model_new.restype = C.c_void_p
    L.tb_host_model_new.argtypes = [C.c_void_p]
    L.tb_host_model_free.argtypes = [C.c_void_p]
    for f in ("accuracy", "mintemp", "maxtemp"):
        getattr(L, f"tb_host_{f}").restype = C.c_double
    L.tb_host_gci.argtypes = [C.c_void_p, C.c_void_p]
    L.tb_host_combine64.restype = C.c_double
    for f in ("exp", "log"):
        getattr(L, f"tb_host_{f}").restype = C.c_double
        getattr(L, f"tb_host_{f}").argtypes = [C.c_double]
    L.tb_host_combine64.argtypes = [C.c_void_p]
    L.tb_host_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tb_host_rates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.tb_host_residuals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    assert L.tb_host_nptrs() == len(INPUTS) + len(OUTPUTS) + 1
    _LIBS[preset] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HostModel:
    """the x86 build's view of a model (keeps the model alive with it)"""

    def __init__(self, model: abi.Model, preset: str = "classic"):
        self.model, self.L = model, lib(preset)
        self.h = C.c_void_p(self.L.tb_host_model_new(C.cast(model.ref(), C.c_void_p)))
        self.accuracy, self.mintemp, self.maxtemp = self.L.tb_host_accuracy(), self.L.tb_host_mintemp(), self.L.tb_host_maxtemp()
        m = model
        self.n, self.ni, self.ne = int(m["npts_nonempty"]), int(m["nions"]), int(m["nelements"])
        self.g, self.nl = int(m["nbfcontinua_ground"]), int(m["nlevels"])

    def __del__(self):
        if getattr(self, "h", None):
            self.L.tb_host_model_free(self.h)

    def gci(self):
        out = np.zeros(self.ni, np.int32)
        self.L.tb_host_gci(self.h, _p(out))
        return out

    def outputs(self) -> dict:
        n, ni, g = self.n, self.ni, self.g
        return dict(renorm=np.zeros(max(n * g, 1)), gamma=np.zeros(max(n * g, 1)), U=np.zeros(n * ni, np.float32), Te=np.zeros(n, np.float32),
                    nne=np.zeros(n, np.float32), Te_solved=np.zeros(n), bracket=np.zeros(2 * n), evals=np.zeros(n, np.int32),
                    flags=np.zeros(n, np.int32), rates=np.zeros(n * abi.THERMAL_NRATES), ground=np.zeros(n * ni, np.float32), phi=np.zeros(n * ni))

    def _pack(self, ins: dict, out: dict, rates_Te=None):
        """the call's arrays, contiguous and typed (kept alive by the returned list), and the three argument blocks"""
        keep = []
        for k in INPUTS:
            v = ins.get(k)
            keep.append(None if v is None else np.ascontiguousarray(v, dtype=_DTYPES.get(k, np.float32)).reshape(-1))
        keep += [out[k] for k in OUTPUTS]
        keep.append(None if rates_Te is None else np.ascontiguousarray(rates_Te, dtype=np.float32))
        ptrs = (C.c_void_p * len(keep))(*[None if a is None else a.ctypes.data for a in keep])
        d = np.array([ins["prev_mid"], ins["tmin"], ins["deltat"]], np.float64)
        iv = np.array([ins.get("nprocs", 1)], np.int32)
        return keep, ptrs, d, iv

    def _shape(self, out: dict) -> dict:
        n, ni, g = self.n, self.ni, self.g
        r = dict(out)
        for k in ("U", "ground", "phi"):
            r[k] = out[k].reshape(n, ni)
        for k in ("renorm", "gamma"):
            r[k] = out[k][: n * g].reshape(n, g)
        r["bracket"] = out["bracket"].reshape(n, 2)
        r["rates"] = out["rates"].reshape(n, abi.THERMAL_NRATES)
        return r

    def solve(self, ins: dict, nthreads: int = 16) -> dict:
        """artis_amd_thermal_solve by the x86 rules: the outputs under thermal_host.cc's names, shaped per cell; "_raw": the flat arrays
        (what rates(rebalance=True) and residuals() read U and gamma from)"""
        out = self.outputs()
        keep, ptrs, d, iv = self._pack(ins, out)
        self.L.tb_host_solve(self.h, ptrs, _p(d), _p(iv), nthreads)
        r = self._shape(out)
        r["_raw"] = out
        return r

    def rates(self, ins: dict, Te=None, rebalance: bool = False, solved: dict = None, nthreads: int = 16) -> dict:
        out = self.outputs()
        if solved is not None:
            out["U"][:], out["gamma"][:] = solved["_raw"]["U"], solved["_raw"]["gamma"]
        keep, ptrs, d, iv = self._pack(ins, out, Te)
        self.L.tb_host_rates(self.h, ptrs, _p(d), _p(iv), int(bool(rebalance)), nthreads)
        return self._shape(out)

    def residuals(self, ins: dict, solved: dict, c: int, T) -> np.ndarray:
        """heating - cooling of cell c (with the ion balance of every evaluation) at the temperatures T"""
        out = self.outputs()
        out["U"][:], out["gamma"][:] = solved["_raw"]["U"], solved["_raw"]["gamma"]
        keep, ptrs, d, iv = self._pack(ins, out)
        T = np.ascontiguousarray(T, np.float64)
        res = np.zeros(len(T))
        self.L.tb_host_residuals(self.h, ptrs, _p(d), _p(iv), int(c), len(T), _p(T), _p(res))
        return res


def combine64(p) -> float:
    a = np.array(p, np.float64)
    assert a.shape == (64,)
    return lib().tb_host_combine64(_p(a))


def resident_inputs(model: abi.Model, state: dict) -> dict:
    """the res_* arrays of a call from a cell state (dict over artis_cellstate's fields)"""
    g = int(model["nbfcontinua_ground"])
    return dict(res_TJ=state["TJ"], res_TR=state["TR"], res_W=state["W"], res_Te=state["Te"], res_nne=state["nne"],
                res_ground=state["ion_groundlevelpops"], res_U=state["ion_partfuncts"],
                res_renorm=np.asarray(state["corrphotoionrenorm"], np.float64) if g else np.zeros(1))


def heating_from_cooling(rates, nl: int, seed: int = 5) -> dict:
    """Synthetic bfheatingcoeffs [ncell, nlevels] and deposition rates [ncell] from the rates [ncell, 10] of every cell at its resident
    T_e (with the ion balance there) formed with bfheatingcoeffs = 1 and no deposition: C0 the cell's cooling, H1 its bound-free heating
    per unit coefficient. Bound-free heating becomes about 0.3 C0, deposition 0.7 C0 x 10^u with u in [-0.4, 0.4] in seven of ten
    cells (a root within a factor two of the resident T_e), far below in the next 15 % (cooling wins everywhere or the root is damped
    from below) and far above in the last (damped from above, or heating wins everywhere)."""
    r = np.asarray(rates, np.float64)
    n = r.shape[0]
    rng = np.random.default_rng(seed)
    C0 = r[:, 0] + r[:, 1] + r[:, 2] + r[:, 3]
    H1 = np.where(r[:, 5] > 0, r[:, 5], 1.0)
    bfheat = (0.3 * C0 / H1)[:, None] * 10.0 ** rng.uniform(-0.3, 0.3, (n, nl))
    kind = rng.random(n)
    u = np.where(kind < 0.7, rng.uniform(-0.4, 0.4, n), np.where(kind < 0.85, rng.uniform(-5.0, -1.0, n), rng.uniform(1.0, 6.0, n)))
    dep = 0.7 * C0 * 10.0 ** u
    bfheat *= np.where(u < -0.4, 10.0 ** u, 1.0)[:, None]  # (a cell that is to lose has little of either)
    alpha = np.where(rng.random(n) < 0.5, 0.1, 0.0) * dep
    return dict(bfheat=bfheat, ntlepton_dep=dep - alpha, dep_alpha=alpha, dep_spfission=np.where(rng.random(n) < 0.25, 0.01, 0.0) * dep)


def probe_inputs(n: int, nl: int) -> dict:
    """the heating inputs heating_from_cooling's rates are formed with"""
    return dict(bfheat=np.ones((n, nl)), ntlepton_dep=np.zeros(n), dep_alpha=np.zeros(n), dep_spfission=np.zeros(n))


def heating_inputs(hm: HostModel, ins: dict, seed: int = 5) -> dict:
    """heating_from_cooling for the inputs `ins` (everything but the heating inputs), the probe's rates by the x86 rules. Only the
    inputs are made this way: what the finder does with them is checked against the rules."""
    probe = dict(ins, **probe_inputs(hm.n, hm.nl))
    r = hm.rates(probe, Te=np.asarray(ins["res_Te"], np.float32), rebalance=True, solved=hm.solve(probe))["rates"]
    return heating_from_cooling(r, hm.nl, seed)

WIDTH = 0.05


def next_timestep(model: abi.Model, ts: abi.Timestep) -> abi.Timestep:
    return synth.make_timestep(ts.c.start + ts.c.width, width_frac=WIDTH, vmax=model["vmax"], nts=ts.c.nts + 1)


def build_model(gridtype: int = abi.GRID_CARTESIAN3D, thick_below_v: float = 1e9):
    """the tests' model: synth "small" on 8 cells per axis with a thick core, so that fitted and unfitted cells mix"""
    model, cs, ts, aux = synth.build("small", ncoord=8, gridtype=gridtype, thick_below_v=thick_below_v, nts=10)
    return synth.with_meannucmass(model), cs, ts, aux


def call_inputs(model: abi.Model, state: dict, ts: abi.Timestep, nm: dict, fit: dict, gamma_raw, ff_raw, col_raw, vol) -> dict:
    """every input of a solve but the heating inputs: the resident state, the fit (TJ, Te, flags), the new matter nm, the raw estimators"""
    ins = resident_inputs(model, state)
    ins.update(fit_TJ=fit["TJ"], fit_Te=fit["Te"], fit_flags=fit["flags"], rho=nm["rho"], massfrac=nm["elem_massfracs"], meanweight=None,
               clump=state["clumpfactor"], gamma_raw=gamma_raw, ff_raw=ff_raw, col_raw=col_raw, assocvol=vol, prev_mid=ts.c.mid,
               tmin=float(model["tmin"]), deltat=ts.c.width, nprocs=1)
    return ins


def synthetic_case(gridtype: int = abi.GRID_CARTESIAN3D, seed: int = 3) -> dict:
    """A whole call without a device: the model's cell state as the resident one, a synthetic fit (T_J two per cent up, the cells that are
    not THICK fitted), synthetic raw estimators (a normalised gamma estimator of 1e-6 .. 1e-2 per second, heating estimators of 1e-12
    erg/s/cm3) and heating_inputs; "solved": the x86 rules' result"""
    model, cs, ts, aux = build_model(gridtype)
    state = dict(cs.d)
    hm = HostModel(model)
    n, g = hm.n, hm.g
    vol = synth.assocvolume_tmin(model)
    ts_next = next_timestep(model, ts)
    nm = synth.next_matter(model, abi.CellState(state), ts.c.mid, ts_next.c.mid, "classic")
    rng = np.random.default_rng(seed)
    enf = 1 / (np.asarray(vol, np.float64) * (ts.c.mid / float(model["tmin"])) ** 3) / ts.c.width
    fitted = np.asarray(state["thick"]) != CELL_THICK
    TJ = np.asarray(state["TJ"], np.float32) * np.float32(1.02)
    fit = dict(TJ=TJ, Te=np.where(fitted, np.asarray(state["Te"], np.float32), TJ), flags=fitted.astype(np.int32) * abi.RADFIELD_FITTED)
    ins = call_inputs(model, state, ts, nm, fit, (10.0 ** rng.uniform(-6, -2, (n, g))) / (enf / H)[:, None], 1e-12 / enf, 1e-12 / enf, vol)
    ins.update(heating_inputs(hm, ins))
    return dict(model=model, state=state, ts=ts, ts_next=ts_next, nm=nm, vol=vol, hm=hm, ins=ins, fitted=fitted, solved=hm.solve(ins))


def damped(T_solved, T_old, mintemp: float, maxtemp: float):
    """the damping of call_T_e_finder (thermalbalance.cc:312-326) of one cell, in doubles"""
    T, T_old = float(T_solved), float(T_old)
    if T > 2 * T_old:
        return min(2 * T_old, maxtemp)
    if T < 0.5 * T_old:
        return max(0.5 * T_old, mintemp)
    return T


def certificate(hm: HostModel, ins: dict, solved: dict, out: dict, cells) -> None:
    """the finder's promise for the bracketed cells of `out` (a download or the rules' own result), by the x86 residual at out's bracket:
    a sign change (or a zero) over [a, b], b - a <= accuracy x min(|a|, |b|) unless the search ran out of evaluations, and T_e the float
    of the damped midpoint"""
    for c in cells:
        a, b = (float(x) for x in out["bracket"][c])
        fa, fb = hm.residuals(ins, solved, c, [a, b])
        assert fa * fb <= 0, (c, a, b, fa, fb)
        if not out["flags"][c] & abi.THERMAL_MAXIT:
            assert abs(a - b) <= hm.accuracy * min(abs(a), abs(b)), (c, a, b)
        assert out["Te_solved"][c] == 0.5 * (a + b), c
        assert out["Te"][c] == np.float32(damped(out["Te_solved"][c], ins["res_Te"][c], hm.mintemp, hm.maxtemp)), c


def dump_call(hm: HostModel, ins: dict, path: str) -> None:
    """the binary form tests/thermal_host/rows_main.cc reads: the model (its struct and every array with the place of its pointer) and
    one call's pointers in thermal_host.cc's order, outputs included"""
    import struct

    m = hm.model
    with open(path, "wb") as f:
        f.write(struct.pack("<q", C.sizeof(abi.CModel)))
        f.write(bytes(m.c))
        patches = []
        for name, ctype, npdt in abi._MODEL_FIELDS:
            if npdt is None or npdt == "i3" or name not in m.d:
                continue
            off = getattr(abi.CModel, name).offset
            if npdt == "p3":
                patches += [(off + 8 * k, m.d[name][k]) for k in range(3)]
            else:
                patches.append((off, m.d[name]))
        f.write(struct.pack("<q", len(patches)))
        for off, arr in patches:
            b = np.ascontiguousarray(arr).tobytes()
            f.write(struct.pack("<qq", off, len(b)))
            f.write(b)
        keep, _, d, iv = hm._pack(ins, hm.outputs())
        f.write(struct.pack("<q", len(keep)))
        for a in keep:
            if a is None:
                f.write(struct.pack("<q", -1))
            else:
                b = a.tobytes()
                f.write(struct.pack("<q", len(b)))
                f.write(b)
        f.write(d.tobytes())
        f.write(struct.pack("<q", int(iv[0])))
