"""Shared by tests/test_photoion_rules.py and tests/test_gpu_photoion.py: the x86 build of artis_amd/csrc/photoion.h
(tests/photoion_host, made on first use) applied to a cell state, and the tests' models, cell states and edge cells."""
import ctypes as C
import os

import numpy as np

import host_build
import thermal_common as tc
from artis_amd import abi, synth

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTDIR = os.path.join(HERE, "photoion_host")
TBMATH, LIBM = 0, 1  # the Math policy of a harness call
PRESETS = ("nltenebular", "ci_nebular_limitbfest")
NTS = 13  # at or above FIRST_NLTE_RADFIELD_TIMESTEP (12; 7 in the CI option sets) and DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP (13)
NTS_EARLY = 3  # below FIRST_NLTE_RADFIELD_TIMESTEP of both presets: the dilute black body
SRC_ESTIMATOR, SRC_INTEGRAL = abi.PHOTOION_SRC_ESTIMATOR, abi.PHOTOION_SRC_INTEGRAL
# the order of the pointers a call hands over (photoion_host.cc enum Ptr)
INPUTS = ("Te", "nne", "clumpfactor", "TR", "W", "levelpops", "radfieldbin_W", "radfieldbin_T_R", "bfrate_normed")
OUTPUTS = ("coeff", "source", "flags", "totals")
_DTYPES = dict(levelpops=np.float64)
_LIBS = {}
_STATES = {}


def lib(preset: str = "nltenebular"):
    if preset in _LIBS:
        return _LIBS[preset]
    L = host_build.load(HOSTDIR, lambda p: f"libphotoion_host_{p}.so", preset)
    L.pi_host_model_new.restype = C.c_void_p
    L.pi_host_model_new.argtypes = [C.c_void_p]
    L.pi_host_model_free.argtypes = [C.c_void_p]
    L.pi_host_sizes.argtypes = [C.c_void_p, C.c_void_p]
    L.pi_host_conts.argtypes = [C.c_void_p, C.c_void_p]
    L.pi_host_bin_consts.argtypes = [C.c_void_p]
    L.pi_host_tepow.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.pi_host_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert L.pi_host_nptrs() == len(INPUTS) + len(OUTPUTS)
    _LIBS[preset] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def mintemp_maxtemp(preset: str):
    table = abi.CI_PRESETS[preset][2] if preset in abi.CI_PRESETS else synth.OPTION_TABLES[preset]
    return float(table[1]), float(table[2])


def state(preset: str, kind: str = "small", ncoord: int = 3):
    """synth.build(kind, ncoord, options=preset) at timestep NTS: (model, cell-state dict without corrphotoioncoeff, the host's
    corrphotoioncoeff, aux); made once, never changed"""
    key = (preset, kind, ncoord)
    if key not in _STATES:
        model, cs, ts, aux = synth.build(kind, ncoord=ncoord, options=preset, nts=NTS)
        cells = {k: v for k, v in cs.d.items() if k != "corrphotoioncoeff"}
        _STATES[key] = (model, cells, cs.d["corrphotoioncoeff"], aux)
    return _STATES[key]


def timestep(model: abi.Model, aux: dict, nts: int = NTS) -> abi.Timestep:
    return synth.make_timestep(aux["t"], width_frac=0.05, vmax=model["vmax"], nts=nts)


def cellstate(cells: dict, **changed) -> abi.CellState:
    return abi.CellState({**cells, **changed})


def seeded_bfrate(ncell: int, nbfestim: int, seed: int = 77) -> np.ndarray:
    """prev_bfrate_normed [ncell, nbfestim] float32: positive rates, every 11th entry negative (no estimate: the integral is taken)"""
    rng = np.random.default_rng(seed)
    bf = (10 ** rng.uniform(-6.0, 0.0, (ncell, max(nbfestim, 1)))).astype(np.float32)
    bf.reshape(-1)[5::11] = -1.0
    return bf[:, :nbfestim]


class HostModel:
    """the x86 build's view of a model (keeps the model alive with it)"""

    def __init__(self, m: abi.Model, preset: str = "nltenebular"):
        self.model, self.L, self.preset = m, lib(preset), preset
        self.h = C.c_void_p(self.L.pi_host_model_new(C.cast(m.ref(), C.c_void_p)))
        sizes = np.zeros(10, np.int64)
        self.L.pi_host_sizes(self.h, _p(sizes))
        (self.n, self.nentries, self.ncont, self.nbfestim, self.nlevels, self.nbins, self.multibin, self.detailed_bf, self.first_nlte,
         self.lut) = (int(v) for v in sizes)
        self.conts = np.zeros((max(self.ncont, 1), 4), np.int32)  # level, target, entry, estimator index
        self.L.pi_host_conts(self.h, _p(self.conts))
        self.conts = self.conts[: self.ncont]
        self.bin_consts = np.zeros(3)
        self.L.pi_host_bin_consts(_p(self.bin_consts))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.pi_host_model_free(self.h)

    def tepow(self, Te) -> np.ndarray:
        Te = np.ascontiguousarray(Te, np.float32)
        out = np.zeros(len(Te))
        self.L.pi_host_tepow(_p(Te), len(Te), _p(out))
        return out

    def outputs(self) -> dict:
        n = max(self.n * self.nentries, 1)
        return dict(coeff=np.full(n, np.nan), source=np.full(n, 255, np.uint8), flags=np.full(max(self.n, 1), -1, np.int32),
                    totals=np.zeros(abi.PHOTOION_NTOTALS, np.int64))

    def _pack(self, ins: dict, out: dict):
        """the call's arrays, contiguous and typed (kept alive by the returned list), and the argument blocks"""
        keep = []
        for k in INPUTS:
            v = ins.get(k)
            keep.append(None if v is None else np.ascontiguousarray(v, dtype=_DTYPES.get(k, np.float32)).reshape(-1))
        keep += [out[k] for k in OUTPUTS]
        ptrs = (C.c_void_p * len(keep))(*[None if a is None else a.ctypes.data for a in keep])
        d = np.array([int(bool(ins.get("use_bf_estimators", 0))), ins.get("nts", NTS), 0.0], np.float64)
        iv = np.array([ins.get("nthreads", 4)], np.int32)
        return keep, ptrs, d, iv

    def compute(self, ins: dict, math: int = TBMATH, nthreads: int = 16) -> dict:
        """artis_amd_set_cellstate_photoion's computation by the x86 rules: coeff and source [ncell, nphixstargets_total], flags [ncell],
        totals as a dict over abi.PHOTOION_TOTALS"""
        out = self.outputs()
        keep, ptrs, d, iv = self._pack(ins, out)
        self.L.pi_host_compute(self.h, ptrs, _p(d), math, nthreads)
        n, ne = self.n, self.nentries
        return dict(coeff=out["coeff"][: n * ne].reshape(n, ne), source=out["source"][: n * ne].reshape(n, ne), flags=out["flags"][:n],
                    totals={k: int(out["totals"][i]) for i, k in enumerate(abi.PHOTOION_TOTALS)})


def call_inputs(cells: dict, use_bf_estimators: bool = False, bfrate_normed=None, nts: int = NTS) -> dict:
    ins = {k: cells.get(k) for k in INPUTS}
    ins.update(bfrate_normed=bfrate_normed if use_bf_estimators else None, use_bf_estimators=use_bf_estimators, nts=nts)
    return ins


def dump_call(hm: HostModel, ins: dict, path: str) -> None:
    """the binary form tests/photoion_host/rows_main.cc reads (tests/thermal_common.py dump_call's, with this harness's pointers)"""
    tc.dump_call(hm, ins, path)


def same_result(a: dict, b: dict, label) -> None:
    """coefficients, sources and flags byte for byte, the totals equal"""
    for k in ("coeff", "source", "flags"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k, int((a[k].view(np.uint8) != b[k].view(np.uint8)).sum()))
    assert a["totals"] == b["totals"], (label, a["totals"], b["totals"])


# ---- edge cells: cell k of the 19-cell state carries edge k; every other cell stays as synth made it
EDGE_ALL_BINS_EMPTY, EDGE_NNLEVEL_ZERO, EDGE_UPPER_INF, EDGE_RATIO_HUGE, EDGE_TE_MIN, EDGE_TE_MAX, EDGE_POP_NAN = range(7)
EDGE_TE_NAN = 7  # (edge_cells(bad=True) only: the one input that gives a non-finite coefficient)


def upper_levels(model: abi.Model, hm: HostModel) -> np.ndarray:
    """the unique level index of every continuum's upper level"""
    m = model
    uls = np.asarray(m["ion_uniquelevelindexstart"])
    out = []
    for ul, t, _, _ in hm.conts:
        ui = int(np.searchsorted(uls, ul, side="right")) - 1
        out.append(int(uls[ui + 1]) + int(m["allphixstargets_levelindex"][int(m["level_phixstargetstart"][ul]) + t]))
    return np.array(out)


def edge_cells(model: abi.Model, cells: dict, hm: HostModel, bad: bool = False) -> dict:
    """the cell-state dict with the edge cells set. Finite and unflagged, all of them, unless bad: then cell EDGE_TE_NAN has T_e = NaN.
    (A NaN level population cannot make a coefficient non-finite: as a lower population it fails nnlevel > 0 and the ratio is 1, as an upper
    one the ratio is not finite and becomes 0 -- ratecoeff.cc:503-507. It is kept as an edge that must stay finite.)"""
    n, nl, nb = hm.n, hm.nlevels, hm.nbins
    mintemp, maxtemp = mintemp_maxtemp(hm.preset)
    pops = np.array(cells["levelpops"], np.float64).reshape(n, nl)
    binW = np.array(cells["radfieldbin_W"], np.float32).reshape(n, nb)
    Te = np.array(cells["Te"], np.float32)
    binW[EDGE_ALL_BINS_EMPTY] = -1.0
    pops[EDGE_NNLEVEL_ZERO] = 0.0
    pops[EDGE_UPPER_INF, np.unique(upper_levels(model, hm))] = np.inf
    # every level of an element's k-th ion 1e44 times the level below's ion: ratios of order 1e30
    level_ion = np.searchsorted(np.asarray(model["ion_uniquelevelindexstart"]), np.arange(nl), side="right") - 1
    ion_in_elem = level_ion - np.asarray(model["elem_uniqueionindexstart"])[np.asarray(model["ion_element"])[level_ion]]
    pops[EDGE_RATIO_HUGE] = 1e-100 * 1e44 ** ion_in_elem.astype(np.float64)
    Te[EDGE_TE_MIN] = mintemp
    Te[EDGE_TE_MAX] = maxtemp
    pops[EDGE_POP_NAN] = np.nan
    if bad:
        Te[EDGE_TE_NAN] = np.nan
    return {**cells, "levelpops": pops.ravel(), "radfieldbin_W": binW.ravel(), "Te": Te}
