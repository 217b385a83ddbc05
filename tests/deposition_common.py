"""Shared by tests/test_deposition_rules.py and tests/test_gpu_deposition.py: the x86 build of artis_amd/csrc/deposition.h
(tests/deposition_host, made on first use, one library per options preset), its bodies applied to host arrays, and the networks and
grids both files use."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:  # run as a script (the networks for deposition_host/rows_main.cc)
    sys.path.insert(0, os.path.dirname(HERE))

import decay_common as dc  # noqa: E402
import host_build  # noqa: E402
from artis_amd import abi, synth  # noqa: E402

HOSTDIR = os.path.join(HERE, "deposition_host")
DAY, EPS, T_MODEL = dc.DAY, dc.EPS, dc.T_MODEL
NETWORKS = ("small", "small_nohe4", "medium")
_LIBS = {}


def lib(preset: str = "classic"):
    if preset in _LIBS:
        return _LIBS[preset]
    L = host_build.load(HOSTDIR, lambda p: f"libdeposition_host_{p}.so", preset)
    L.dep_host_last_error.restype = C.c_char_p
    L.dep_host_validate.restype = C.c_char_p
    L.dep_host_validate.argtypes = [C.POINTER(abi.DepositionModel), C.c_int, C.c_int64]
    L.dep_host_new.restype = C.c_void_p
    L.dep_host_new.argtypes = [C.POINTER(abi.DecayModel), C.POINTER(abi.DepositionModel), C.c_int64]
    L.dep_host_free.argtypes = [C.c_void_p]
    L.dep_host_nrad.argtypes = [C.c_void_p]
    L.dep_host_rows.argtypes = [C.c_void_p] * 5
    L.dep_host_vectors.argtypes = [C.c_void_p] * 4
    L.dep_host_vectors_validate.restype = C.c_char_p
    L.dep_host_vectors_validate.argtypes = [C.c_void_p] * 2
    L.dep_host_totmass.argtypes = [C.c_void_p] * 2
    L.dep_host_cells.argtypes = [C.c_void_p] * 11 + [C.c_int, C.c_int]
    L.dep_host_totals.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    _LIBS[preset] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def depth() -> int:
    """DEP_DEPTH of the rule header"""
    return int(lib().dep_host_depth())


def validate(em: dict, nnuclides: int, ncell: int) -> str:
    m, keep = abi.deposition_model(em)
    return lib().dep_host_validate(C.byref(m), nnuclides, ncell).decode()


def step_params(model, t_mid, prev_mid, prev_width, nts_next, num_grey, thick, thick_vpkt=0.0, nprocs=1) -> np.ndarray:
    """the flat form of artis_dep::Step that dep_host_cells reads"""
    return np.array([t_mid, float(model["tmin"]), float(model["rmax"]), prev_mid, prev_width, nprocs, nts_next, num_grey, thick, thick_vpkt], np.float64)


class HostDep:
    """the x86 build's rows and bodies over a decay model and a deposition model (dicts over the structs' fields) of a grid"""

    def __init__(self, dm: dict, em: dict, model: abi.Model, preset: str = "classic"):
        self.L = lib(preset)
        self.n, self.nn, self.np = int(model["npts_nonempty"]), len(dm["nuc_z"]), len(dm["path_start"]) - 1
        d, keep_d = abi.decay_model(dm)
        m, keep_m = abi.deposition_model(em)
        h = self.L.dep_host_new(C.byref(d), C.byref(m), self.n)
        assert h, self.L.dep_host_last_error().decode()
        self.h = C.c_void_p(h)
        self.nrad = int(self.L.dep_host_nrad(self.h))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.dep_host_free(self.h)

    def rows(self) -> dict:
        out = dict(top_start=np.zeros(self.nn + 1, np.int32), top_path=np.zeros(max(self.np, 1), np.int32), top_end=np.zeros(max(self.np, 1), np.int32),
                   rad_nuc=np.zeros(max(self.nrad, 1), np.int32))
        self.L.dep_host_rows(self.h, *[_p(out[k]) for k in ("top_start", "top_path", "top_end", "rad_nuc")])
        out["top_path"], out["top_end"], out["rad_nuc"] = out["top_path"][: self.np], out["top_end"][: self.np], out["rad_nuc"][: self.nrad]
        return out

    def vectors(self, coeffs: dict) -> np.ndarray:
        out = np.zeros((abi.DEP_NVECTORS, self.nn))
        c = [np.ascontiguousarray(coeffs[k], np.float64) for k in ("endnuc_coeff", "survivingfrac")]
        self.L.dep_host_vectors(self.h, _p(c[0]), _p(c[1]), _p(out))
        return out

    def vectors_validate(self, vectors) -> str:
        v = np.ascontiguousarray(vectors, np.float64)
        return self.L.dep_host_vectors_validate(self.h, _p(v)).decode()

    def totmass(self):
        """(totmassnuclide, mtot)"""
        out = np.zeros(self.nn + 1)
        self.L.dep_host_totmass(self.h, _p(out))
        return out[:-1].copy(), float(out[-1])

    def cells(self, step: np.ndarray, vectors, rho, kappagrey, raw, all_nuclides: bool = False, nthreads: int = 8) -> dict:
        """raw: [4, ncell] the raw estimators {gamma, positron, electron, alpha}"""
        n = self.n
        out = dict(eps_ana=np.zeros((abi.DEP_NCHANNELS, n)), dep=np.zeros((abi.DEP_NCHANNELS, n)), ntlepton_deposition_rate_density=np.zeros(n),
                   grey_depth=np.zeros(n, np.float32), thick=np.zeros(n, np.int32))
        v, r, k, e = (np.ascontiguousarray(vectors, np.float64), np.ascontiguousarray(rho, np.float32), np.ascontiguousarray(kappagrey, np.float32),
                      np.ascontiguousarray(raw, np.float64))
        assert v.shape == (abi.DEP_NVECTORS, self.nn) and e.shape == (4, n) and r.shape == k.shape == (n,)
        self.L.dep_host_cells(self.h, _p(np.ascontiguousarray(step, np.float64)), _p(v), _p(r), _p(k), _p(e),
                              *[_p(out[x]) for x in ("eps_ana", "dep", "ntlepton_deposition_rate_density", "grey_depth", "thick")],
                              int(all_nuclides), nthreads)
        return out

    def totals(self, nprocs: int, vectors, raw, totmass) -> np.ndarray:
        out = np.zeros(abi.DEP_NTOTALS)
        v, e, t = np.ascontiguousarray(vectors, np.float64), np.ascontiguousarray(raw, np.float64), np.ascontiguousarray(totmass, np.float64)
        self.L.dep_host_totals(self.h, int(nprocs), _p(v), _p(e), _p(t), _p(out))
        return out


def raw_estimators(n: int, seed: int = 5) -> np.ndarray:
    """[4, n] synthetic raw deposition estimators [erg] {gamma, positron, electron, alpha}; a few cells saw no packet"""
    rng = np.random.default_rng(seed)
    raw = 10.0 ** rng.uniform(38.0, 42.0, (4, n))
    raw[:, rng.random(n) < 0.1] = 0.0
    return raw


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for kind in NETWORKS:
        dc.dump_network(synth.decay_network(kind), [14, 26, 27], os.path.join(sys.argv[1], kind + ".txt"))
