"""ctypes binding of the test-only host emulation of the kernel bodies (tests/hostemu)."""
import ctypes as C
import os

import numpy as np

import host_build
from artis_amd import abi

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu")
_LIBS = {}


def lib(preset: str = "classic", only_this: bool = False):
    if preset not in _LIBS:
        L = host_build.load(_HERE, lambda p: "libartis_hostemu.so" if p == "classic" else f"libartis_hostemu_{p}.so", preset, only_this)
        L.artis_emu_update_packets.restype = C.c_int
        L.artis_emu_update_packets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]
        L.artis_emu_cellcache.restype = C.c_int
        _LIBS[preset] = L
    return _LIBS[preset]


def update_packets(model, cells, ts, packets, est, budget=4, preset="classic"):
    rc = lib(preset).artis_emu_update_packets(C.cast(model.ref(), C.c_void_p), C.cast(cells.ref(), C.c_void_p),
                                        C.cast(ts.ref(), C.c_void_p), abi.packets_ptr(packets), len(packets),
                                        C.cast(est.ref(), C.c_void_p), budget)
    if rc != 0:
        raise RuntimeError(f"kernel-body emulation raised error flag {rc}")


def _main_arrays(d):
    return {
        "levelpops": np.zeros(d["nlevels"]), "maprocessrates": np.zeros(d["nlevels"] * 9),
        "matrans": np.zeros(max(d["nmatransblock"], 1)), "allcont_nnlevel": np.zeros(max(d["nbfcontinua"], 1)),
        "allcont_departure": np.zeros(max(d["nbfcontinua"], 1)), "allcont_edgepart": np.zeros(max(d["nbfcontinua"], 1)),
        "allcont_keepbits": np.zeros((d["nbfcontinua"] + 63) // 64 + 1, dtype=np.uint64),
        "corrphotoioncoeff": np.zeros(max(d["nphixstargets_total"], 1)), "cooling_contrib": np.zeros(max(d["ncoolingterms"], 1)),
        "ion_cooling_contribs": np.zeros(d["nions"]),
    }


def cellcache(model, cells, ts, c, preset="classic"):
    out = _main_arrays(model.d)
    chi = C.c_double(0.0)
    args = [C.cast(model.ref(), C.c_void_p), C.cast(cells.ref(), C.c_void_p), C.cast(ts.ref(), C.c_void_p), C.c_int(c)] + \
           [v.ctypes.data_as(C.c_void_p) for v in out.values()] + [C.byref(chi)]
    rc = lib(preset).artis_emu_cellcache(*args)
    if rc != 0:
        raise RuntimeError("emulated populate raised an error flag")
    out["chi_ff_nnionpart"] = chi.value
    return out


class CellCacheView:
    """The emulation's rows of every cell, populated once (artis_emu_cc_open), with the two views the engine has: debug_cellcache(c), the
    reference's spans, and debug_cellcache_array(c, name), one array of the row as stored (abi.CC_ARRAYS). error: the population's flag."""

    def __init__(self, model, cells, ts, preset="classic"):
        self.model, self.cells, self.ts, self.L = model, cells, ts, lib(preset)  # (kept alive: the rows point into them)
        self.L.artis_emu_cc_open.restype = C.c_void_p
        self.L.artis_emu_cc_close.argtypes = [C.c_void_p]
        self.L.artis_emu_cc_array.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        err = C.c_int(0)
        self.h = C.c_void_p(self.L.artis_emu_cc_open(C.cast(model.ref(), C.c_void_p), C.cast(cells.ref(), C.c_void_p),
                                                     C.cast(ts.ref(), C.c_void_p), C.byref(err)))
        self.error = err.value

    def close(self):
        if getattr(self, "h", None):
            self.L.artis_emu_cc_close(self.h)
            self.h = None

    __del__ = close

    def debug_cellcache(self, c):
        out = _main_arrays(self.model.d)
        chi = C.c_double(0.0)
        rc = self.L.artis_emu_cc_main(self.h, C.c_int(c), *[v.ctypes.data_as(C.c_void_p) for v in out.values()], C.byref(chi))
        if rc != 0:
            raise RuntimeError(f"emulated populate raised error flag {rc}")
        out["chi_ff_nnionpart"] = chi.value
        return out

    def debug_cellcache_array(self, c, which):
        idx, dtype, width = abi.CC_ARRAYS[which]
        need = C.c_int64(0)
        probe = np.zeros(1, dtype=np.uint8)
        self.L.artis_emu_cc_array(self.h, int(c), idx, probe.ctypes.data_as(C.c_void_p), 0, C.byref(need))
        if need.value <= 0:
            raise KeyError(f"{which}: no such array in this build or model")
        buf = np.zeros(need.value // np.dtype(dtype).itemsize, dtype=dtype)
        written = C.c_int64(0)
        rc = self.L.artis_emu_cc_array(self.h, int(c), idx, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(written))
        assert rc == 0 and written.value == buf.nbytes, (which, rc, written.value)
        return buf.reshape(-1, 2) if width == 2 else buf


def cool_guide_row(model, ion_cooling_contribs, cooling_contrib):
    """the row of cooling guides physics.h cool_guide_entry() gives for these two cumulative lists (tables.h "COOLING GUIDES"), uint16. The
    guides depend on no build option, so the classic library serves every build (and is the only one made for it)."""
    L = lib("classic", only_this=True)
    L.artis_emu_cool_guide_row.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    a = np.ascontiguousarray(ion_cooling_contribs, dtype=np.float64)
    b = np.ascontiguousarray(cooling_contrib, dtype=np.float64)
    n = L.artis_emu_cool_guide_row(C.cast(model.ref(), C.c_void_p), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), None, 0)
    out = np.zeros(max(n, 1), dtype=np.uint16)
    L.artis_emu_cool_guide_row(C.cast(model.ref(), C.c_void_p), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                               out.ctypes.data_as(C.c_void_p), n)
    return out[:n]
