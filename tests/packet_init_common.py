"""Shared by tests/test_packet_init_rules.py and tests/test_gpu_packet_init.py: the x86 build of artis_amd/csrc/packet_init.h
(tests/packet_init_host, made on first use), its bodies applied to host arrays, and the networks, grids and set-ups both files use."""
import ctypes as C
import functools
import os

import numpy as np

import decay_common as dc
import host_build
from artis_amd import abi, synth

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTDIR = os.path.join(HERE, "packet_init_host")
DAY, T_MODEL = dc.DAY, dc.T_MODEL
TMAX = 80.0 * DAY  # (tmin of the grids is 2 days, t_model 1 day)
SEED_BASE = 20240611  # of every population here
_LIB = []


def lib():
    if _LIB:
        return _LIB[0]
    L = host_build.load(HOSTDIR, lambda p: f"libpacket_init_host_{p}.so", "classic")
    L.pinit_host_last_error.restype = C.c_char_p
    L.pinit_host_lerp.restype = L.pinit_host_std_lerp.restype = C.c_double
    L.pinit_host_lerp.argtypes = L.pinit_host_std_lerp.argtypes = [C.c_double] * 3
    L.pinit_host_validate.restype = C.c_char_p
    L.pinit_host_validate.argtypes = [C.POINTER(abi.PacketInitModel), C.c_int, C.c_int64, C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_int)]
    L.pinit_host_vector_validate.restype = C.c_char_p
    L.pinit_host_vector_validate.argtypes = [C.c_void_p, C.c_int]
    L.pinit_host_new.restype = C.c_void_p
    L.pinit_host_new.argtypes = [C.c_void_p, C.POINTER(abi.DecayModel), C.POINTER(abi.DepositionModel), C.POINTER(abi.PacketInitModel)]
    L.pinit_host_free.argtypes = [C.c_void_p]
    L.pinit_host_energy.argtypes = [C.c_void_p] * 2
    L.pinit_host_cells.restype = C.c_double
    L.pinit_host_cells.argtypes = [C.c_void_p] * 4 + [C.c_int]
    L.pinit_host_channel.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_int]
    L.pinit_host_run.argtypes = [C.c_void_p, C.c_int64, C.c_uint32] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_int]
    _LIB.append(L)
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def stride() -> int:
    """CKPT_STRIDE of the rule header"""
    return int(lib().pinit_host_stride())


def validate(pm: dict, nuc_meanlife, ncell: int, tmin: float, t_model: float):
    """(text, unsupported) of packet_init_validate"""
    m, keep = abi.packet_init_model(pm)
    life = np.ascontiguousarray(nuc_meanlife, np.float64)
    u = C.c_int(0)
    text = lib().pinit_host_validate(C.byref(m), len(life), ncell, _p(life), tmin, t_model, C.byref(u)).decode()
    return text, bool(u.value)


class HostPinit:
    """the x86 build's bodies over a decay model, a deposition model and a pellet model (dicts over the structs' fields) of a grid"""

    def __init__(self, dm: dict, em: dict, pm: dict, model: abi.Model):
        self.L = lib()
        self.n, self.ngrid, self.np = int(model["npts_nonempty"]), int(model["ngrid"]), len(dm["path_start"]) - 1
        d, keep_d = abi.decay_model(dm)
        m, keep_m = abi.deposition_model(em)
        q, keep_q = abi.packet_init_model(pm)
        h = self.L.pinit_host_new(C.cast(model.ref(), C.c_void_p), C.byref(d), C.byref(m), C.byref(q))
        assert h, self.L.pinit_host_last_error().decode()
        self.h = C.c_void_p(h)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.pinit_host_free(self.h)

    def energy(self) -> np.ndarray:
        out = np.zeros(max(self.np, 1))
        self.L.pinit_host_energy(self.h, _p(out))
        return out[: self.np]

    def cells(self, E, nthreads: int = 8) -> dict:
        """endecay_per_mass, en_cumulative, etot_simtime with the vector E; the checkpoints stay in the harness for channel() and run()"""
        E = np.ascontiguousarray(E, np.float64)
        assert E.shape == (self.np,)
        out = dict(endecay_per_mass=np.zeros(self.n), en_cumulative=np.zeros(self.ngrid))
        out["etot_simtime"] = float(self.L.pinit_host_cells(self.h, _p(E), _p(out["endecay_per_mass"]), _p(out["en_cumulative"]), nthreads))
        return out

    def channel(self, cell: int, u: float, full: bool = False) -> int:
        return int(self.L.pinit_host_channel(self.h, cell, np.float32(u), int(full)))

    def run(self, npackets: int, seed_base: int = SEED_BASE, budget: int = 0, max_calls: int = 1 << 30, margins: bool = False, nthreads: int = 8) -> dict:
        """the population after cells(): packets, channel, trials, the scalars, "calls" (pellet_decay calls of the slowest packet; -1: one
        was not complete after max_calls) and, with margins, tdecay_unit and margin per packet (packet_init_host.cc)"""
        out = dict(packets=np.zeros(npackets, abi.PACKET_DTYPE), channel=np.zeros(npackets, np.int32), trials=np.zeros(npackets, np.int32))
        if margins:
            out.update(tdecay_unit=np.zeros(npackets), margin=np.zeros(npackets))
        scal = np.zeros(4)
        out["calls"] = int(self.L.pinit_host_run(self.h, npackets, seed_base & 0xFFFFFFFF, _p(out["packets"]), _p(out["channel"]), _p(out["trials"]), _p(scal),
                                                 budget or int(self.L.pinit_host_default_trials()), max_calls, _p(out.get("tdecay_unit")), _p(out.get("margin")),
                                                 nthreads))
        out.update(etot_simtime=scal[0], e_cmf_per_packet=scal[1], e_cmf_total=scal[2], e_ratio=scal[3])
        return out


def grid(gridtype):
    """(model, cs, ts, aux): decay_common's 8^3 grid and 5 shells, and a 6 x 12 cylindrical grid (the 3D and 2D ones have empty cells)"""
    if gridtype == abi.GRID_CYLINDRICAL2D:
        return synth.build("small", ncoord=6, gridtype=abi.GRID_CYLINDRICAL2D)
    return dc.grid(gridtype)


@functools.lru_cache(maxsize=None)
def case(gridtype: int, kind: str, initial_energy: bool):
    """(model, cs, ts, dm, em, pm) of a grid, a network of synth.decay_network and the initial-energy channel on or off. In cell
    ZERO_CELL no nuclide of the network has any mass and the cell has no initial energy: it must receive no pellet."""
    model, cs, ts, aux = grid(gridtype)
    net = synth.decay_network(kind)
    dm = synth.decay_model(model, cs, aux, net, t_model=T_MODEL)
    em = synth.deposition_model(model, net)
    pm = synth.packet_init_model(model, net, em, TMAX, initial_energy=initial_energy)
    zc = ZERO_CELL % int(model["npts_nonempty"])
    dm["initnucmassfrac"] = np.array(dm["initnucmassfrac"], np.float32)
    dm["initnucmassfrac"][zc, :] = 0.0
    if initial_energy:
        pm["initenergyq"][zc] = 0.0
    return model, cs, ts, dm, em, pm


ZERO_CELL = 1  # synth.decay_model's zero_cell


def propcell_of(model: abi.Model, c: int) -> int:
    """the propagation cell of non-empty cell c"""
    return int(np.nonzero(np.asarray(model["propcell_nonemptymgi"]) == c)[0][0])
