"""Shared by tests/test_ion_balance_rules.py and tests/test_gpu_ion_balance.py: the x86 build of artis_amd/csrc/ion_balance.h
(tests/ionbal_host, made on first use) and its per-cell balance applied to host arrays."""
import ctypes as C
import os

import numpy as np

import host_build
from artis_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTDIR = os.path.join(HERE, "ionbal_host")
H = 6.6260755e-27
CELL_THICK = 1  # ARTIS_CELL_THICK
_LIBS = {}


def lib(preset: str = "classic"):
    if preset in _LIBS:
        return _LIBS[preset]
    L = host_build.load(HOSTDIR, lambda p: f"libionbal_host_{p}.so", preset)
    L.ib_host_model_new.restype = C.c_void_p
    L.ib_host_model_new.argtypes = [C.c_void_p]
    L.ib_host_model_free.argtypes = [C.c_void_p]
    L.ib_host_minpop.restype = C.c_double
    L.ib_host_temperature_grid.argtypes = [C.c_void_p, C.c_void_p]
    L.ib_host_alpha_sp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ib_host_ion_spontrecombcoeff.restype = C.c_double
    L.ib_host_ion_spontrecombcoeff.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float]
    L.ib_host_balance.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 18 + [C.c_int]
    L.ib_host_residual.restype = C.c_double
    L.ib_host_residual.argtypes = [C.c_void_p, C.c_float] + [C.c_void_p] * 7 + [C.c_double, C.c_void_p]
    _LIBS[preset] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HostModel:
    """the x86 build's view of a model (keeps the model alive with it)"""

    def __init__(self, model: abi.Model, preset: str = "classic"):
        self.model, self.L = model, lib(preset)
        self.h = C.c_void_p(self.L.ib_host_model_new(C.cast(model.ref(), C.c_void_p)))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ib_host_model_free(self.h)

    def temperature_grid(self):
        out = np.zeros(self.L.ib_host_tablesize() + 1)
        self.L.ib_host_temperature_grid(self.h, _p(out))
        return out

    def alpha_sp(self):
        ni = int(self.model["nions"])
        a = np.zeros(ni * self.L.ib_host_tablesize(), np.float32)
        gci = np.zeros(ni, np.int32)
        self.L.ib_host_alpha_sp(self.h, _p(a), _p(gci))
        return a.reshape(ni, -1), gci

    def balance(self, TJ, Te, forced, ground_cur, massfrac, meanweight, rho, clump, gamma, nthreads: int = 8) -> dict:
        m = self.model
        n, ni, ne = int(m["npts_nonempty"]), int(m["nions"]), int(m["nelements"])
        f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
        ins = dict(TJ=f32(TJ), Te=f32(Te), forced=np.ascontiguousarray(forced, np.int32), ground_cur=f32(ground_cur),
                   massfrac=f32(massfrac), meanweight=None if meanweight is None else f32(meanweight), rho=f32(rho), clump=f32(clump),
                   gamma=np.ascontiguousarray(gamma, np.float64).reshape(-1) if np.size(gamma) else np.zeros(1))
        out = dict(nnetot=np.zeros(n, np.float32), U=np.zeros(n * ni, np.float32), phi=np.zeros(n * ni), uppermost=np.zeros(n * ne, np.int32),
                   ground=np.zeros(n * ni, np.float32), nne=np.zeros(n, np.float32), nne_root=np.zeros(n, np.float32),
                   evals=np.zeros(n, np.int32), flags=np.zeros(n, np.int32))
        self.L.ib_host_balance(self.h, n, *[_p(ins[k]) for k in ("TJ", "Te", "forced", "ground_cur", "massfrac", "meanweight", "rho", "clump",
                                                              "gamma")],
                               *[_p(out[k]) for k in ("nnetot", "U", "phi", "uppermost", "ground", "nne", "nne_root", "evals", "flags")], nthreads)
        for k in ("U", "phi", "ground"):
            out[k] = out[k].reshape(n, ni)
        out["uppermost"] = out["uppermost"].reshape(n, ne)
        return out

    def residual(self, rho, massfrac, meanweight, U, phi, gamma, gci, uppermost, nne):
        f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
        fl = np.zeros(1, np.int32)
        args = [f32(massfrac), None if meanweight is None else f32(meanweight), f32(U), np.ascontiguousarray(phi, np.float64),
                np.ascontiguousarray(gamma, np.float64) if np.size(gamma) else np.zeros(1), np.ascontiguousarray(gci, np.int32),
                np.ascontiguousarray(uppermost, np.int32)]
        r = self.L.ib_host_residual(self.h, float(rho), *[_p(a) for a in args], float(nne), _p(fl))
        return r, int(fl[0])


def gamma_normed(gamma_raw, assocvol, prev_mid: float, tmin: float, deltat: float, nprocs: int = 1):
    """the engine's normalisation of the raw gamma estimator [ncell, nbfg] (update_grid.cc:358 with radfield_fit.h
    cell_normfactors): the same IEEE operations in the same order"""
    r = prev_mid / tmin
    deltaV = np.asarray(assocvol, np.float64) * (r * r * r)
    enf = 1 / deltaV / deltat / nprocs
    return np.asarray(gamma_raw, np.float64) * (enf / H)[:, None]
