"""Shared by tests/test_ratecoeff_rules.py and tests/test_gpu_ratecoeff.py: the x86 build of artis_amd/csrc/ratecoeff_tables.h
(tests/ratecoeff_host, made on first use) applied to a model, and the tests' models."""
import ctypes as C
import os

import numpy as np

import host_build
import thermal_common as tc
from artis_amd import abi, synth

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTDIR = os.path.join(HERE, "ratecoeff_host")
TBMATH, LIBM = 0, 1  # the Math policy of a harness call
TABLES = ("spontrecombcoeffs", "corrphotoioncoeffs", "bfcooling_coeffs")
TOTALS = ("integrals", "nodes", "at_depth_cap", "flagged")
_LIBS = {}
_MODELS = {}


def lib(preset: str = "classic"):
    if preset in _LIBS:
        return _LIBS[preset]
    L = host_build.load(HOSTDIR, lambda p: f"libratecoeff_host_{p}.so", preset)
    L.rc_host_model_new.restype = C.c_void_p
    L.rc_host_model_new.argtypes = [C.c_void_p]
    L.rc_host_model_free.argtypes = [C.c_void_p]
    L.rc_host_sizes.argtypes = [C.c_void_p, C.c_void_p]
    L.rc_host_conts.argtypes = [C.c_void_p, C.c_void_p]
    L.rc_host_tgrid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rc_host_gk61_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rc_host_tables.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    _LIBS[preset] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def model(preset: str = "classic", kind: str = "small", ncoord: int = 6) -> abi.Model:
    """synth.build(kind, ncoord) with the preset's options (made once)"""
    key = (preset, kind, ncoord)
    if key not in _MODELS:
        _MODELS[key] = synth.build(kind, ncoord=ncoord, options=preset)
    return _MODELS[key][0]


def changed(m: abi.Model, **arrays) -> abi.Model:
    """a copy of the model with some of its arrays replaced"""
    return abi.Model({**m.d, **arrays})


def gk61_tables(preset: str = "classic"):
    """x[31], w[31], wg[15] as the integrator holds them"""
    x, w, wg = np.zeros(31), np.zeros(31), np.zeros(15)
    lib(preset).rc_host_gk61_tables(_p(x), _p(w), _p(wg))
    return x, w, wg


class HostModel:
    """the x86 build's view of a model (keeps the model alive with it)"""

    def __init__(self, m: abi.Model, preset: str = "classic"):
        self.model, self.L, self.preset = m, lib(preset), preset
        self.h = C.c_void_p(self.L.rc_host_model_new(C.cast(m.ref(), C.c_void_p)))
        sizes = np.zeros(5, np.int64)
        self.L.rc_host_sizes(self.h, _p(sizes))
        self.nbf, self.tablesize, self.ntables, self.ncovered, listed = (int(v) for v in sizes)
        assert listed
        self.conts = np.zeros((max(self.nbf, 1), 2), np.int32)
        self.L.rc_host_conts(self.h, _p(self.conts))
        self.conts = self.conts[: self.nbf]
        self.tgrid, self.Tpow = np.zeros(self.tablesize), np.zeros(self.tablesize)
        self.L.rc_host_tgrid(self.h, _p(self.tgrid), _p(self.Tpow))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.rc_host_model_free(self.h)

    def tables(self, math: int = TBMATH, shared: bool = True, nthreads: int = 16) -> dict:
        """artis_amd_ratecoeff_compute by the x86 rules: the tables and flags as [nbfcontinua, TABLESIZE] (corrphotoioncoeffs None in a
        build without USE_LUT_PHOTOION) and the totals as a dict over TOTALS"""
        shape = (self.nbf, self.tablesize)
        n = max(self.nbf * self.tablesize, 1)
        spont, cool, flags, totals = np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1, np.int32), np.zeros(4, np.int64)
        gamma = np.full(n, np.nan) if self.ntables == 3 else None
        self.L.rc_host_tables(self.h, math, int(shared), nthreads, _p(spont), _p(gamma), _p(cool), _p(flags), _p(totals))
        cut = lambda a: None if a is None else a[: shape[0] * shape[1]].reshape(shape)
        return dict(spontrecombcoeffs=cut(spont), corrphotoioncoeffs=cut(gamma), bfcooling_coeffs=cut(cool), flags=cut(flags),
                    totals={k: int(totals[i]) for i, k in enumerate(TOTALS)})

    # the call has no arrays besides the model's: tests/thermal_common.py dump_call writes the model and these
    def outputs(self) -> dict:
        return {}

    def _pack(self, ins: dict, out: dict):
        return [], None, np.zeros(3), np.array([ins.get("nthreads", 4)], np.int32)


def dump_call(hm: HostModel, path: str, nthreads: int = 4) -> None:
    """the binary form tests/ratecoeff_host/rows_main.cc reads"""
    tc.dump_call(hm, dict(nthreads=nthreads), path)


def same_tables(a: dict, b: dict, label) -> None:
    """every table and the flags byte for byte, the totals equal"""
    for k in TABLES + ("flags",):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (label, k)
            continue
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k, int((a[k] != b[k]).sum()))
