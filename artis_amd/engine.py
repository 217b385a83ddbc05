"""Python host side over the C-ABI of libartis_amd.so (ctypes; no torch types cross the boundary).

Mirrors the reference's call sequence for one timestep:
    update_grid()      -> Engine.set_cellstate(cells, ts)       (cell cache populated on the GPU)
    update_packets()   -> Engine.update_packets(packets, est)   (host buffers)  or the device-resident
                          upload_packets / step / download_packets calls used by bench.py
    reduce_estimators  -> Engine.estimators_devptr() handed to an RCCL all-reduce by the caller
The library has no CPU path: creating an Engine without a HIP device raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi
from .build import SO, build, so_path


class EngineError(RuntimeError):
    pass


_LIBS = {}


def load_library(build_if_missing: bool = False, preset: str = "classic"):
    """Load the engine built for an options preset (include/artis_options.h). One library per preset."""
    if preset in _LIBS:
        return _LIBS[preset]
    so = so_path(preset)
    so = os.environ.get("ARTIS_AMD_SO" if preset == "classic" else f"ARTIS_AMD_SO_{preset.upper()}", so)  # A/B builds (tuning only)
    if not os.path.exists(so):
        if not build_if_missing:
            raise EngineError(f"{so} is missing: run `python -m artis_amd.build` (hipcc, gfx950). There is no CPU fallback.")
        build(preset=preset)
    L = C.CDLL(so)
    L.artis_amd_last_error.restype = C.c_char_p
    L.artis_amd_abi_version.restype = C.c_int
    L.artis_amd_sizeof_packet.restype = C.c_size_t
    L.artis_amd_engine_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.artis_amd_engine_create_ex.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.Config), C.POINTER(C.c_void_p)]
    L.artis_amd_engine_config.argtypes = [C.c_void_p, C.POINTER(abi.Config)]
    L.artis_amd_engine_plan.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.Config), C.c_int64, C.POINTER(abi.Plan)]
    L.artis_amd_config_default.argtypes = [C.POINTER(abi.Config)]
    L.artis_amd_config_default.restype = None
    L.artis_amd_sizeof_config.restype = C.c_size_t
    L.artis_amd_sizeof_plan.restype = C.c_size_t
    L.artis_amd_engine_destroy.argtypes = [C.c_void_p]
    L.artis_amd_engine_destroy.restype = None
    L.artis_amd_set_cellstate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.artis_amd_populate_cellcache.argtypes = [C.c_void_p, C.c_void_p]
    L.artis_amd_update_packets.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.artis_amd_packets_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.artis_amd_packets_download.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.artis_amd_packets_snapshot.argtypes = [C.c_void_p]
    L.artis_amd_packets_restore.argtypes = [C.c_void_p]
    L.artis_amd_update_packets_device.argtypes = [C.c_void_p, C.c_void_p]
    L.artis_amd_estimators_zero.argtypes = [C.c_void_p, C.c_void_p]
    L.artis_amd_estimators_download.argtypes = [C.c_void_p, C.c_void_p]
    L.artis_amd_estimators_devptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.artis_amd_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.artis_amd_spectra_compute.argtypes = [C.c_void_p, C.POINTER(abi.SpectraConfig), C.c_void_p]
    L.artis_amd_spectra_devptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.artis_amd_spectra_download.argtypes = [C.c_void_p, C.POINTER(abi.Spectra)]
    L.artis_amd_radfield_fit.argtypes = [C.c_void_p, C.POINTER(abi.RadfieldConfig), C.c_void_p]
    L.artis_amd_radfield_download.argtypes = [C.c_void_p, C.POINTER(abi.Radfield)]
    L.artis_amd_grid_update.argtypes = [C.c_void_p, C.POINTER(abi.GridUpdate), C.c_void_p, C.c_void_p]
    L.artis_amd_grid_update_download.argtypes = [C.c_void_p, C.POINTER(abi.GridUpdateResult)]
    L.artis_amd_decay_setup.argtypes = [C.c_void_p, C.POINTER(abi.DecayModel)]
    L.artis_amd_decay_update.argtypes = [C.c_void_p, C.c_double, C.POINTER(abi.DecayCoeffs), C.c_int, C.c_void_p]
    L.artis_amd_decay_download.argtypes = [C.c_void_p, C.POINTER(abi.DecayResult)]
    L.artis_amd_grid_update_decayed.argtypes = [C.c_void_p, C.POINTER(abi.GridUpdate), C.c_void_p, C.c_void_p]
    L.artis_amd_deposition_setup.argtypes = [C.c_void_p, C.POINTER(abi.DepositionModel)]
    L.artis_amd_deposition_update.argtypes = [C.c_void_p, C.POINTER(abi.DepositionParams), C.c_void_p]
    L.artis_amd_deposition_download.argtypes = [C.c_void_p, C.POINTER(abi.DepositionResult)]
    L.artis_amd_deposition_devptr.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.artis_amd_grid_update_deposited.argtypes = [C.c_void_p, C.POINTER(abi.GridUpdate), C.c_void_p, C.c_void_p]
    L.artis_amd_packet_init_setup.argtypes = [C.c_void_p, C.POINTER(abi.PacketInitModel)]
    L.artis_amd_packet_init.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p]
    L.artis_amd_packet_init_download.argtypes = [C.c_void_p, C.POINTER(abi.PacketInitResult)]
    L.artis_amd_initial_state.argtypes = [C.c_void_p, C.POINTER(abi.InitialParams), C.c_void_p]
    L.artis_amd_initial_state_download.argtypes = [C.c_void_p, C.POINTER(abi.InitialResult)]
    L.artis_amd_grid_update_initial.argtypes = [C.c_void_p, C.POINTER(abi.GridUpdate), C.c_void_p, C.c_void_p]
    L.artis_amd_thermal_solve.argtypes = [C.c_void_p, C.POINTER(abi.ThermalParams), C.c_void_p]
    L.artis_amd_thermal_rates.argtypes = [C.c_void_p, C.POINTER(abi.ThermalParams), C.c_void_p, C.c_int, C.c_void_p]
    L.artis_amd_thermal_download.argtypes = [C.c_void_p, C.POINTER(abi.ThermalResult)]
    L.artis_amd_grid_update_thermal.argtypes = [C.c_void_p, C.POINTER(abi.GridUpdate), C.c_void_p, C.c_void_p]
    L.artis_amd_bfheating_update.argtypes = [C.c_void_p, C.POINTER(abi.BfheatingParams), C.c_void_p]
    L.artis_amd_bfheating_download.argtypes = [C.c_void_p, C.POINTER(abi.BfheatingResult)]
    L.artis_amd_thermal_solve_bfheated.argtypes = [C.c_void_p, C.POINTER(abi.ThermalParams), C.c_void_p]
    L.artis_amd_debug_gk61.argtypes = [C.c_int32, C.POINTER(abi.Gk61Case), C.POINTER(abi.Gk61Result)]
    L.artis_amd_ratecoeff_compute.argtypes = [C.c_void_p, C.POINTER(abi.RatecoeffRequest)]
    L.artis_amd_ratecoeff_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.RatecoeffStats)]
    L.artis_amd_set_cellstate_photoion.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(abi.PhotoionParams), C.c_void_p]
    L.artis_amd_photoion_download.argtypes = [C.c_void_p, C.POINTER(abi.PhotoionResult)]
    if L.artis_amd_abi_version() != abi.ABI_VERSION:  # a stale or foreign build would read these ctypes structs with another layout
        raise EngineError(f"{so}: ABI version {L.artis_amd_abi_version()}, this package describes version {abi.ABI_VERSION}")
    assert L.artis_amd_sizeof_packet() == abi.PACKET_DTYPE.itemsize
    assert L.artis_amd_sizeof_config() == C.sizeof(abi.Config) and L.artis_amd_sizeof_plan() == C.sizeof(abi.Plan)
    L.artis_amd_options_preset.restype = C.c_char_p
    assert L.artis_amd_options_preset().decode() == preset, (L.artis_amd_options_preset(), preset)
    _LIBS[preset] = L
    return L


EXPORTED_SYMBOLS = [
    "artis_amd_last_error", "artis_amd_abi_version", "artis_amd_sizeof_packet", "artis_amd_engine_create",
    "artis_amd_engine_destroy", "artis_amd_set_cellstate", "artis_amd_update_packets", "artis_amd_packets_upload",
    "artis_amd_packets_download", "artis_amd_packets_snapshot", "artis_amd_packets_restore",
    "artis_amd_update_packets_device", "artis_amd_estimators_zero", "artis_amd_estimators_download",
    "artis_amd_estimators_devptr", "artis_amd_last_kernel_ms", "artis_amd_debug_cellcache", "artis_amd_debug_sort_list", "artis_amd_debug_visit_counts", "artis_amd_last_kernel_ms_by_kind",
    "artis_amd_populate_cellcache",
    "artis_amd_last_kernel_breakdown",
    "artis_amd_last_kernel_launches",
    "artis_amd_last_kernel_table",
    "artis_amd_options_preset",
    "artis_amd_allreduce_estimators", "artis_amd_comm_unique_id", "artis_amd_comm_init", "artis_amd_comm_count",
    "artis_amd_cache_tiles", "artis_amd_last_tiling", "artis_amd_last_tiling_fills", "artis_amd_last_tiling_parked", "artis_amd_last_pool_resets", "artis_amd_record_tiers", "artis_amd_last_thermal_variants", "artis_amd_last_estimator_forms", "artis_amd_last_pool_usage", "artis_amd_last_absent_records",
    "artis_amd_spectra_compute", "artis_amd_spectra_devptr", "artis_amd_spectra_download",
    "artis_amd_radfield_fit", "artis_amd_radfield_download",
    "artis_amd_grid_update", "artis_amd_grid_update_download",
    "artis_amd_decay_setup", "artis_amd_decay_update", "artis_amd_decay_download", "artis_amd_grid_update_decayed",
    "artis_amd_deposition_setup", "artis_amd_deposition_update", "artis_amd_deposition_download", "artis_amd_deposition_devptr",
    "artis_amd_grid_update_deposited",
    "artis_amd_packet_init_setup", "artis_amd_packet_init", "artis_amd_packet_init_download",
    "artis_amd_initial_state", "artis_amd_initial_state_download", "artis_amd_grid_update_initial",
    "artis_amd_thermal_solve", "artis_amd_thermal_rates", "artis_amd_thermal_download", "artis_amd_grid_update_thermal",
    "artis_amd_bfheating_update", "artis_amd_bfheating_download", "artis_amd_thermal_solve_bfheated", "artis_amd_debug_gk61",
    "artis_amd_ratecoeff_compute", "artis_amd_ratecoeff_download",
    "artis_amd_set_cellstate_photoion", "artis_amd_photoion_download",
    "artis_amd_sizeof_config", "artis_amd_config_default", "artis_amd_engine_create_ex", "artis_amd_engine_config",
    "artis_amd_sizeof_plan", "artis_amd_engine_plan",
    "artis_amd_debug_cellcache_array",
]


def _as_config(config) -> abi.Config:
    """an abi.Config, or a dict of its fields (the others at "automatic / default")"""
    return config if isinstance(config, abi.Config) else abi.config(**config)


def plan(model: abi.Model, config=None, device: int = 0, preset: str = "classic", free_bytes: int = 0) -> dict:
    """The layout Engine(model, device, preset, config) would choose, without building it (artis_amd_engine_plan): a dict over the fields of
    artis_amd_plan. free_bytes = 0 asks the device for its free memory; a value given is taken instead and no device is needed."""
    L = load_library(preset=preset)
    out = abi.Plan(struct_size=C.sizeof(abi.Plan))
    cfg = C.byref(_as_config(config)) if config is not None else None
    rc = L.artis_amd_engine_plan(C.cast(model.ref(), C.c_void_p), device, cfg, int(free_bytes), C.byref(out))
    if rc != 0:
        raise EngineError(f"artis_amd error {rc}: {L.artis_amd_last_error().decode()}")
    return abi.struct_dict(out)


def debug_gk61(cases, preset: str = "classic") -> list:
    """artis_amd_debug_gk61: the adaptive 61-point Gauss-Kronrod integrator on the analytic integrands of tests/golden/gk61_reference.json,
    on the current device, one lane per case. cases: (which, p, a, b, tol); returns a dict per case (result, error, evals, nodes, maxdepth)."""
    L = load_library(preset=preset)
    n = len(cases)
    arr = (abi.Gk61Case * max(n, 1))(*[abi.Gk61Case(which=int(w), p=float(p), a=float(a), b=float(b), tol=float(tol)) for w, p, a, b, tol in cases])
    out = (abi.Gk61Result * max(n, 1))()
    rc = L.artis_amd_debug_gk61(n, arr, out)
    if rc != 0:
        raise EngineError(f"artis_amd error {rc}: {L.artis_amd_last_error().decode()}")
    return [{k: getattr(out[i], k) for k, _ in abi.Gk61Result._fields_} for i in range(n)]


class Engine:
    def __init__(self, model: abi.Model, device: int = 0, preset: str = "classic", config=None):
        """config: an abi.Config (abi.config(...)) or a dict of its fields -- how the engine uses its device (include/artis_amd.h
        artis_amd_config: a field set there wins over its ARTIS_AMD_* variable); None: artis_amd_engine_create, the variables and defaults."""
        self.L = load_library(preset=preset)
        self.model = model
        self.h = C.c_void_p()
        if config is None:
            self._check(self.L.artis_amd_engine_create(C.cast(model.ref(), C.c_void_p), device, C.byref(self.h)))
        else:
            self._check(self.L.artis_amd_engine_create_ex(C.cast(model.ref(), C.c_void_p), device, C.byref(_as_config(config)), C.byref(self.h)))

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(f"artis_amd error {rc}: {self.L.artis_amd_last_error().decode()}")

    def close(self):
        if self.h:
            self.L.artis_amd_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_cellstate(self, cells: abi.CellState, ts: abi.Timestep):
        self._cells, self._ts = cells, ts
        self._check(self.L.artis_amd_set_cellstate(self.h, C.cast(cells.ref(), C.c_void_p), C.cast(ts.ref(), C.c_void_p)))

    def populate_cellcache(self, stream: int = 0):
        self._check(self.L.artis_amd_populate_cellcache(self.h, C.c_void_p(stream)))

    def update_packets(self, packets: np.ndarray, est: abi.Estimators):
        """Host-buffer form of the reference's update_packets() (update_packets.cc:530)."""
        self._check(self.L.artis_amd_update_packets(self.h, abi.packets_ptr(packets), len(packets), C.cast(est.ref(), C.c_void_p)))

    # device-resident form
    def upload_packets(self, packets: np.ndarray):
        self._check(self.L.artis_amd_packets_upload(self.h, abi.packets_ptr(packets), len(packets)))

    def download_packets(self, packets: np.ndarray):
        self._check(self.L.artis_amd_packets_download(self.h, abi.packets_ptr(packets), len(packets)))

    def snapshot(self):
        self._check(self.L.artis_amd_packets_snapshot(self.h))

    def restore(self):
        self._check(self.L.artis_amd_packets_restore(self.h))

    def step(self, stream: int = 0):
        self._check(self.L.artis_amd_update_packets_device(self.h, C.c_void_p(stream)))

    def zero_estimators(self, stream: int = 0):
        self._check(self.L.artis_amd_estimators_zero(self.h, C.c_void_p(stream)))

    def download_estimators(self, est: abi.Estimators):
        self._check(self.L.artis_amd_estimators_download(self.h, C.cast(est.ref(), C.c_void_p)))

    def estimators_devptr(self):
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.L.artis_amd_estimators_devptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # emergent spectra and light curves of the resident packets (include/artis_amd.h artis_amd_spectra_*)
    def spectra_compute(self, ts_start, ts_width, tmin: float, tmax: float, dirbin: int = -1, emission_absorption: bool = False,
                        stokes: bool = False, gamma: bool = False, stream: int = 0):
        starts = np.ascontiguousarray(ts_start, dtype=np.float64)
        widths = np.ascontiguousarray(ts_width, dtype=np.float64)
        if starts.shape != widths.shape or starts.ndim != 1:
            raise EngineError("ts_start and ts_width must be 1-D arrays of one length")
        cfg = abi.SpectraConfig(struct_size=C.sizeof(abi.SpectraConfig), ntimesteps=len(starts), dirbin=dirbin,
                                ts_start=starts.ctypes.data_as(C.POINTER(C.c_double)), ts_width=widths.ctypes.data_as(C.POINTER(C.c_double)),
                                tmin=tmin, tmax=tmax, emission_absorption=int(bool(emission_absorption)), stokes=int(bool(stokes)),
                                gamma=int(bool(gamma)))
        self._check(self.L.artis_amd_spectra_compute(self.h, C.byref(cfg), C.c_void_p(stream)))
        self._spec_cfg = dict(nts=len(starts), all=dirbin == abi.SPEC_ALL_DIRBINS, ea=bool(emission_absorption), stokes=bool(stokes),
                              gamma=bool(gamma))

    def spectra_devptr(self):
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.L.artis_amd_spectra_devptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def spectra_download(self) -> dict:
        c = self._spec_cfg
        info = abi.Spectra(struct_size=C.sizeof(abi.Spectra))
        self._check(self.L.artis_amd_spectra_download(self.h, C.byref(info)))  # shapes and counts first
        T, D, B, P = info.ntimesteps, info.ndirslots, abi.SPEC_MNUBINS, info.proccount
        A = info.nelements * info.max_nions
        lead = (D,) if c["all"] else ()
        shapes = {"lum": lead + (T,), "lumcmf": lead + (T,), "flux": lead + (B, T)}
        if c["stokes"]:
            shapes.update(flux_q=lead + (B, T), flux_u=lead + (B, T))
        if c["ea"]:
            shapes.update(emission=lead + (B, T, P), trueemission=lead + (B, T, P), absorption=lead + (B, T, A))
            if c["stokes"]:
                shapes.update(emission_q=lead + (B, T, P), emission_u=lead + (B, T, P), absorption_q=lead + (B, T, A),
                              absorption_u=lead + (B, T, A))
        if c["gamma"]:
            shapes.update(gamma_lum=(T,), gamma_lumcmf=(T,), gamma_flux=(B, T))
        out = {k: np.zeros(v) for k, v in shapes.items()}
        for k, v in out.items():
            setattr(info, k, v.ctypes.data_as(C.POINTER(C.c_double)))
        grids = {k: np.zeros(abi.SPEC_MNUBINS, dtype=np.float32) for k in ("lower_freq", "delta_freq", "gamma_lower_freq", "gamma_delta_freq")}
        for k, v in grids.items():
            setattr(info, k, v.ctypes.data_as(C.POINTER(C.c_float)))
        self._check(self.L.artis_amd_spectra_download(self.h, C.byref(info)))
        out.update(grids)
        out.update(nescaped=int(info.nescaped_rpkt), nescaped_gamma=int(info.nescaped_gamma), proccount=P,
                   nelements=info.nelements, max_nions=info.max_nions)
        return out

    def spectra(self, ts_start, ts_width, tmin: float, tmax: float, dirbin: int = -1, emission_absorption: bool = False,
                stokes: bool = False, gamma: bool = False) -> dict:
        """The emergent spectra and light curves of the resident packets, binned on the device (tools/exspec.py's keys and the
        reference's layouts: flux[nnu, nts], emission[nnu, nts, column], ...; a leading axis of 1 + MABINS with
        dirbin=abi.SPEC_ALL_DIRBINS: slot 0 the angle average, slot s direction bin s - 1)."""
        self.spectra_compute(ts_start, ts_width, tmin, tmax, dirbin, emission_absorption, stokes, gamma)
        return self.spectra_download()

    # radiation-field fit of the grid update (include/artis_amd.h artis_amd_radfield_*)
    def radfield_fit(self, prev_mid: float, deltat: float, assocvolume_tmin, nprocs: int = 1, lte_iteration: bool = False,
                     bfrate_normed_seed=None, stream: int = 0) -> dict:
        """Fit T_J, T_R, W (and the multibin W, T_R) of every cell to the engine's estimators and cell state on the device, then
        download everything: numpy arrays under the field names of artis_radfield (cell_counts [ncell, 5]), the per-call
        "totals" as a dict over abi.RADFIELD_COUNTS and "kernel_ms" (per-cell, per-bin kernel). assocvolume_tmin: [npts_nonempty]
        (synth.assocvolume_tmin for the synthetic grids)."""
        cfg, keep = abi.radfield_config(prev_mid, deltat, nprocs, assocvolume_tmin, lte_iteration, bfrate_normed_seed)
        self._check(self.L.artis_amd_radfield_fit(self.h, C.byref(cfg), C.c_void_p(stream)))
        del keep
        return self.radfield_download()

    def radfield_download(self) -> dict:
        info = abi.Radfield(struct_size=C.sizeof(abi.Radfield))
        self._check(self.L.artis_amd_radfield_download(self.h, C.byref(info)))  # sizes first
        out = abi.radfield_arrays(info.npts_nonempty, info.nbins, info.nbfestim, info.detailed_linecount)
        abi.radfield_point(info, out)
        self._check(self.L.artis_amd_radfield_download(self.h, C.byref(info)))
        if info.nbins:
            out["radfieldbin_T_R"] = out["radfieldbin_T_R"].reshape(info.npts_nonempty, info.nbins)
            out["radfieldbin_W"] = out["radfieldbin_W"].reshape(info.npts_nonempty, info.nbins)
        out["totals"] = {k: int(info.totals[i]) for i, k in enumerate(abi.RADFIELD_COUNTS)}
        out["kernel_ms"] = (float(info.kernel_ms[0]), float(info.kernel_ms[1]))
        return out

    # ionisation balance and hand-over of the grid update (include/artis_amd.h artis_amd_grid_update*)
    def grid_update(self, ts_next: abi.Timestep, rho, elem_massfracs, thick, use_fit: bool = True, elem_meanweight=None, TJ=None,
                    TR=None, W=None, Te=None, kappagrey=None, clumpfactor=None, ffegrp=None, stream: int = 0) -> dict:
        """Partition functions and ion balance of every cell on the device, from the last radiation-field fit (use_fit) or the host's
        temperatures; the result becomes the engine's cell state for ts_next and the cell cache is filled. Returns the download
        (grid_update_download). A refused state raises EngineError; its flags stay downloadable."""
        u, keep = abi.grid_update_config(use_fit, rho, elem_massfracs, thick, elem_meanweight, TJ, TR, W, Te, kappagrey, clumpfactor,
                                         ffegrp)
        self._ts = ts_next
        self._check(self.L.artis_amd_grid_update(self.h, C.byref(u), C.cast(ts_next.ref(), C.c_void_p), C.c_void_p(stream)))
        del keep
        return self.grid_update_download()

    def grid_update_download(self) -> dict:
        """numpy arrays under the field names of artis_grid_update_result ([ncell, nions] / [ncell, nelements] /
        [ncell, nbfcontinua_ground] for the per-ion, per-element and per-continuum ones), "ncells_flagged" as a dict over
        abi.IONBAL_FLAGS, "total_evals" and "kernel_ms" (gamma + partition functions, phi, per-cell solve, cell-cache fill)."""
        info = abi.GridUpdateResult(struct_size=C.sizeof(abi.GridUpdateResult))
        self._check(self.L.artis_amd_grid_update_download(self.h, C.byref(info)))  # sizes first
        n, ni, ne, g = info.npts_nonempty, info.nions, info.nelements, info.nbfcontinua_ground
        out = abi.grid_update_arrays(n, ni, ne, g)
        types = dict(abi.GridUpdateResult._fields_)
        for k, v in out.items():
            setattr(info, k, v.ctypes.data_as(types[k]))
        self._check(self.L.artis_amd_grid_update_download(self.h, C.byref(info)))
        out["ion_partfuncts"] = out["ion_partfuncts"].reshape(n, ni)
        out["ion_groundlevelpops"] = out["ion_groundlevelpops"].reshape(n, ni)
        out["phi"] = out["phi"].reshape(n, ni)
        out["uppermost_ion"] = out["uppermost_ion"].reshape(n, ne)
        out["gamma_normed"] = out["gamma_normed"][: n * g].reshape(n, g)
        out["ncells_flagged"] = {k: int(info.ncells_flagged[i]) for i, k in enumerate(abi.IONBAL_FLAGS)}
        out["total_evals"] = int(info.total_evals)
        out["kernel_ms"] = tuple(float(x) for x in info.kernel_ms)
        return out

    # decay and abundance update of the grid update (include/artis_amd.h artis_amd_decay_*)
    def decay_setup(self, decay_model: dict):
        """Validate and upload a decay network with the cells' initial composition: a dict over artis_decay_model's fields
        (synth.decay_model). A second call replaces the first."""
        m, keep = abi.decay_model(decay_model)
        self._check(self.L.artis_amd_decay_setup(self.h, C.byref(m)))
        del keep

    def decay_update(self, t_mid: float, coeffs=None, want_nuclides: bool = False, stream: int = 0) -> dict:
        """rho, element mass fractions and mean weights of every cell at t_mid on the device; coeffs: a dict with endnuc_coeff, he4_coeff
        and survivingfrac from the host (used as they are), or None (the device forms them). Returns the download."""
        c, keep = (None, None) if coeffs is None else abi.decay_coeffs(coeffs["endnuc_coeff"], coeffs["he4_coeff"], coeffs["survivingfrac"])
        self._check(self.L.artis_amd_decay_update(self.h, float(t_mid), C.byref(c) if c is not None else None, int(bool(want_nuclides)),
                                                  C.c_void_p(stream)))
        del keep
        return self.decay_download()

    def decay_download(self) -> dict:
        """numpy arrays under the field names of artis_decay_result (elem_* [ncell, nelements], nuc_massfracs [ncell, nnuclides] when the
        update was asked for them), "he4_nucindex", "kernel_ms" (coefficients, cells, nuclides) and "t_mid".
        """
        info = abi.DecayResult(struct_size=C.sizeof(abi.DecayResult))
        self._check(self.L.artis_amd_decay_download(self.h, C.byref(info)))  # sizes first
        n, ne, nn, npaths = info.npts_nonempty, info.nelements, info.nnuclides, info.npaths
        out = abi.decay_arrays(n, ne, nn, npaths, bool(info.have_nuclides))
        types = dict(abi.DecayResult._fields_)
        for k, v in out.items():
            if v.size:
                setattr(info, k, v.ctypes.data_as(types[k]))
        self._check(self.L.artis_amd_decay_download(self.h, C.byref(info)))
        out["elem_massfracs"] = out["elem_massfracs"].reshape(n, ne)
        out["elem_meanweight"] = out["elem_meanweight"].reshape(n, ne)
        if "nuc_massfracs" in out:
            out["nuc_massfracs"] = out["nuc_massfracs"].reshape(n, nn)
        out.update(he4_nucindex=int(info.he4_nucindex), kernel_ms=tuple(float(x) for x in info.kernel_ms), t_mid=float(info.t_mid))
        return out

    def decay_download_times(self):
        """the HIP-event times [ms] of the last decay_update's kernels (coefficients, cells, nuclides), without copying an array"""
        info = abi.DecayResult(struct_size=C.sizeof(abi.DecayResult))
        self._check(self.L.artis_amd_decay_download(self.h, C.byref(info)))
        return tuple(float(x) for x in info.kernel_ms)

    def grid_update_decayed(self, ts_next: abi.Timestep, thick, use_fit: bool = True, TJ=None, TR=None, W=None, Te=None, kappagrey=None,
                            clumpfactor=None, ffegrp=None, stream: int = 0, _matter=None) -> dict:
        """grid_update with rho, elem_massfracs and elem_meanweight of the last decay_update(ts_next.mid), which never leave the device.
        (_matter: (rho, elem_massfracs, elem_meanweight) handed over all the same, which the library refuses: for the tests.)"""
        rho, mf, mw = _matter if _matter is not None else (None, None, None)
        u, keep = abi.grid_update_config(use_fit, rho, mf, thick, mw, TJ, TR, W, Te, kappagrey, clumpfactor, ffegrp)
        self._check(self.L.artis_amd_grid_update_decayed(self.h, C.byref(u), C.cast(ts_next.ref(), C.c_void_p), C.c_void_p(stream)))
        self._ts = ts_next
        del keep
        return self.grid_update_download()

    # deposition rates and thickness of the grid update (include/artis_amd.h artis_amd_deposition_*)
    def deposition_setup(self, deposition_model: dict):
        """Validate and upload the nuclides' decay energies and branch probabilities with the cells' volumes and radial positions: a dict
        over artis_deposition_model's array fields (synth.decay_energies, synth.assocvolume_tmin, synth.radial_pos_tmin). Needs
        decay_setup; a second call replaces the first."""
        m, keep = abi.deposition_model(deposition_model)
        self._check(self.L.artis_amd_deposition_setup(self.h, C.byref(m)))
        del keep

    def deposition_update(self, mid: float, width: float, nts: int, nts_next: int, num_grey_timesteps: int, optical_depth_is_thick: float,
                          optical_depth_is_thick_vpkt: float = 0.0, nprocs: int = 1, power_vectors=None, stream: int = 0) -> dict:
        """Emission powers, deposition rates, grey depth and thickness flag of every cell and the timestep totals on the device, from the
        last decay_update and the estimators of the step (mid, width, nts) just propagated; power_vectors: [11, nnuclides] from the host
        (used as they are), or None (the device forms them). Returns the download."""
        p, keep = abi.deposition_params(mid, width, nts, nts_next, num_grey_timesteps, optical_depth_is_thick, optical_depth_is_thick_vpkt,
                                        nprocs, power_vectors)
        self._check(self.L.artis_amd_deposition_update(self.h, C.byref(p), C.c_void_p(stream)))
        del keep
        return self.deposition_download()

    def deposition_download(self, arrays: bool = True) -> dict:
        """numpy arrays under the field names of artis_deposition_result (eps_ana, dep [5, ncell]; power_vectors [11, nnuclides]), "totals"
        as a dict over abi.DEP_TOTALS, "mtot", "nradioactive", "nts_next", "t_mid" and "kernel_ms" (powers, cells, totals);
        arrays=False: only the reported fields"""
        info = abi.DepositionResult(struct_size=C.sizeof(abi.DepositionResult))
        self._check(self.L.artis_amd_deposition_download(self.h, C.byref(info)))  # sizes first
        n, nn = info.npts_nonempty, info.nnuclides
        out = abi.deposition_arrays(n, nn) if arrays else {}
        types = dict(abi.DepositionResult._fields_)
        for k, v in out.items():
            if v.size:
                setattr(info, k, v.ctypes.data_as(types[k]))
        if arrays:
            self._check(self.L.artis_amd_deposition_download(self.h, C.byref(info)))
            out["eps_ana"] = out["eps_ana"].reshape(abi.DEP_NCHANNELS, n)
            out["dep"] = out["dep"].reshape(abi.DEP_NCHANNELS, n)
            out["power_vectors"] = out["power_vectors"].reshape(abi.DEP_NVECTORS, nn)
        out.update(totals={k: float(info.totals[i]) for i, k in enumerate(abi.DEP_TOTALS)}, mtot=float(info.mtot), nradioactive=int(info.nradioactive),
                   nts_next=int(info.nts_next), t_mid=float(info.t_mid), kernel_ms=tuple(float(x) for x in info.kernel_ms))
        return out

    def grid_update_deposited(self, ts_next: abi.Timestep, use_fit: bool = True, TJ=None, TR=None, W=None, Te=None, kappagrey=None,
                              clumpfactor=None, ffegrp=None, stream: int = 0, _thick=None) -> dict:
        """grid_update_decayed with the thickness flags of the last deposition_update too: no array of the new timestep comes from the
        host. (_thick: flags handed over all the same, which the library refuses: for the tests.)"""
        u, keep = abi.grid_update_config(use_fit, None, None, _thick, None, TJ, TR, W, Te, kappagrey, clumpfactor, ffegrp)
        self._check(self.L.artis_amd_grid_update_deposited(self.h, C.byref(u), C.cast(ts_next.ref(), C.c_void_p), C.c_void_p(stream)))
        self._ts = ts_next
        del keep
        return self.grid_update_download()

    # pellet initialisation (include/artis_amd.h artis_amd_packet_init*)
    def packet_init_setup(self, packet_init_model: dict):
        """Validate and upload the gamma lines, the daughters' probability sums, the cells' initial energy and the switches: a dict over
        artis_packet_init_model's fields (synth.packet_init_model). Needs decay_setup and deposition_setup; a second call replaces the
        first, a new decay or deposition set-up invalidates it."""
        m, keep = abi.packet_init_model(packet_init_model)
        self._check(self.L.artis_amd_packet_init_setup(self.h, C.byref(m)))
        del keep

    def packet_init(self, npackets: int, seed_base: int, energy_vector=None, stream: int = 0) -> dict:
        """Make npackets pellets by the reference's packet_init() on the device and install them as the resident population
        (download_packets returns them in caller order); energy_vector: [npaths] energy_per_massoftopnuc_decaypath from the host (used as
        it is), or None (the device forms it). Returns the download without the per-packet arrays."""
        keep = None if energy_vector is None else np.ascontiguousarray(energy_vector, dtype=np.float64).reshape(-1)
        self._check(self.L.artis_amd_packet_init(self.h, int(npackets), int(seed_base) & 0xFFFFFFFF, keep.ctypes.data_as(C.c_void_p) if keep is not None else None,
                                                 C.c_void_p(stream)))
        del keep
        return self.packet_init_download(per_packet=False)

    def packet_init_download(self, per_packet: bool = True, arrays: bool = True) -> dict:
        """numpy arrays under the field names of artis_packet_init_result (channel and trials [npackets] only with per_packet), the
        reported scalars, "kernel_ms" as a dict over abi.PINIT_KERNELS; arrays=False: only the reported fields"""
        info = abi.PacketInitResult(struct_size=C.sizeof(abi.PacketInitResult))
        self._check(self.L.artis_amd_packet_init_download(self.h, C.byref(info)))  # sizes first
        out = abi.packet_init_arrays(info.ngrid, info.npts_nonempty, info.npaths, info.npackets if per_packet else 0) if arrays else {}
        if not per_packet:
            out.pop("channel", None), out.pop("trials", None)
        types = dict(abi.PacketInitResult._fields_)
        for k, v in out.items():
            if v.size:
                setattr(info, k, v.ctypes.data_as(types[k]))
        if arrays:
            self._check(self.L.artis_amd_packet_init_download(self.h, C.byref(info)))
        for k in ("npackets", "ngrid", "npts_nonempty", "npaths", "ncheckpoints", "continuation_launches", "max_trials"):
            out[k] = int(getattr(info, k))
        for k in ("etot_simtime", "e_cmf_per_packet", "e_cmf_total", "e_ratio"):
            out[k] = float(getattr(info, k))
        out["kernel_ms"] = {k: float(info.kernel_ms[i]) for i, k in enumerate(abi.PINIT_KERNELS)}
        return out

    # initial temperatures and the first cell state (include/artis_amd.h artis_amd_initial_state*)
    def initial_state(self, params: dict, stream: int = 0) -> dict:
        """T_initial, kappagrey, grey depth and thickness flag of every cell before the first timestep, on the device: a dict over
        artis_initial_params's fields (synth.initial_model plus tstart, nts_first, num_grey_timesteps and the depths; energy_vector
        [npaths] from the host, used as it is, or absent: the device forms it). Needs decay_setup, deposition_setup, packet_init_setup
        and a decay_update at tstart. Returns the download."""
        p, keep = abi.initial_params(params)
        self._check(self.L.artis_amd_initial_state(self.h, C.byref(p), C.c_void_p(stream)))
        del keep
        return self.initial_state_download()

    def initial_state_download(self, arrays: bool = True) -> dict:
        """numpy arrays under the field names of artis_initial_result, "ncells_branch" as a dict over abi.INITIAL_BRANCHES, the reported
        scalars, "kernel_ms" as a dict over abi.INITIAL_KERNELS; arrays=False: only the reported fields"""
        info = abi.InitialResult(struct_size=C.sizeof(abi.InitialResult))
        self._check(self.L.artis_amd_initial_state_download(self.h, C.byref(info)))  # sizes first
        out = abi.initial_arrays(info.npts_nonempty, info.npaths) if arrays else {}
        types = dict(abi.InitialResult._fields_)
        for k, v in out.items():
            if v.size:
                setattr(info, k, v.ctypes.data_as(types[k]))
        if arrays:
            self._check(self.L.artis_amd_initial_state_download(self.h, C.byref(info)))
        out["ncells_branch"] = {k: int(info.ncells_branch[i]) for i, k in enumerate(abi.INITIAL_BRANCHES)}
        for k in ("ncells_kappa_invalid", "first_nonfinite_cell", "npts_nonempty", "npaths", "rpkt_grey_type", "nts_first"):
            out[k] = int(getattr(info, k))
        for k in ("first_nonfinite_rho_tmin", "first_nonfinite_endecay", "tstart"):
            out[k] = float(getattr(info, k))
        out["kernel_ms"] = {k: float(info.kernel_ms[i]) for i, k in enumerate(abi.INITIAL_KERNELS)}
        return out

    def grid_update_initial(self, ts_first: abi.Timestep, clumpfactor=None, ffegrp=None, stream: int = 0) -> dict:
        """The first cell state: grid_update with the matter of the last decay_update(ts_first.mid) and the temperatures, W = 1,
        kappagrey and thickness flags of the last initial_state, none of which leaves the device. Needs no set_cellstate before it."""
        u, keep = abi.grid_update_config(False, None, None, None, clumpfactor=clumpfactor, ffegrp=ffegrp)
        self._check(self.L.artis_amd_grid_update_initial(self.h, C.byref(u), C.cast(ts_first.ref(), C.c_void_p), C.c_void_p(stream)))
        self._ts = ts_first
        del keep
        return self.grid_update_download()

    # thermal balance of the thin cells (include/artis_amd.h artis_amd_thermal_*)
    def thermal_solve(self, bfheatingcoeffs, rho=None, elem_massfracs=None, elem_meanweight=None, ntlepton_dep=None, dep_alpha=None,
                      dep_spfission=None, clumpfactor=None, stream: int = 0) -> dict:
        """Renormalisation, Gamma per ground population, partition functions and the T_e of the thermal balance of every cell the last
        radiation-field fit has fitted, on the device. bfheatingcoeffs [ncell, nlevels] from the host; the matter None: the last
        decay_update's; the deposition inputs None: the last deposition_update's. Returns the download."""
        p, keep = abi.thermal_params(bfheatingcoeffs, rho, elem_massfracs, elem_meanweight, ntlepton_dep, dep_alpha, dep_spfission, clumpfactor)
        self._check(self.L.artis_amd_thermal_solve(self.h, C.byref(p), C.c_void_p(stream)))
        del keep
        return self.thermal_download()

    # bound-free heating coefficients of the thin cells (include/artis_amd.h artis_amd_bfheating_*)
    def bfheating_update(self, TR=None, W=None, stream: int = 0) -> dict:
        """The bound-free heating coefficients [ncell, nlevels] of every cell the last radiation-field fit has fitted, renormalised, on
        the device. TR, W [ncell] None: the fit's; given: those instead in the levels' integrals. Returns the download."""
        p, keep = abi.bfheating_params(TR, W)
        self._check(self.L.artis_amd_bfheating_update(self.h, C.byref(p), C.c_void_p(stream)))
        del keep
        return self.bfheating_download()

    def bfheating_download(self, arrays: bool = True) -> dict:
        """"coeffs" [ncell, nlevels], "renorm" [ncell, nbfcontinua_ground], "flags" [ncell] (abi.BFHEAT_*), "totals" as a dict over
        abi.BFHEAT_TOTALS, "nfitted", "nintegrals", "nlevels_with_targets" and "kernel_ms" as a dict over abi.BFHEAT_KERNELS;
        arrays=False: only those"""
        info = abi.BfheatingResult(struct_size=C.sizeof(abi.BfheatingResult))
        self._check(self.L.artis_amd_bfheating_download(self.h, C.byref(info)))  # sizes first
        n, nl, g = info.npts_nonempty, info.nlevels, info.nbfcontinua_ground
        out = {}
        if arrays:
            out = dict(coeffs=np.zeros(max(n * nl, 1)), renorm=np.zeros(max(n * g, 1)), flags=np.zeros(max(n, 1), np.int32))
            types = dict(abi.BfheatingResult._fields_)
            for k, v in out.items():
                setattr(info, k, v.ctypes.data_as(types[k]))
            self._check(self.L.artis_amd_bfheating_download(self.h, C.byref(info)))
            out["coeffs"] = out["coeffs"][: n * nl].reshape(n, nl)
            out["renorm"] = out["renorm"][: n * g].reshape(n, g)
            out["flags"] = out["flags"][:n]
        out.update(totals={k: int(info.totals[i]) for i, k in enumerate(abi.BFHEAT_TOTALS)}, nfitted=int(info.nfitted),
                   nintegrals=int(info.nintegrals), nlevels_with_targets=int(info.nlevels_with_targets),
                   kernel_ms={k: float(info.kernel_ms[i]) for i, k in enumerate(abi.BFHEAT_KERNELS)})
        return out

    def thermal_solve_bfheated(self, rho=None, elem_massfracs=None, elem_meanweight=None, ntlepton_dep=None, dep_alpha=None,
                               dep_spfission=None, clumpfactor=None, stream: int = 0) -> dict:
        """thermal_solve with the coefficients of the last bfheating_update, read where they lie on the device. Returns the download."""
        p, keep = abi.thermal_params(None, rho, elem_massfracs, elem_meanweight, ntlepton_dep, dep_alpha, dep_spfission, clumpfactor)
        self._check(self.L.artis_amd_thermal_solve_bfheated(self.h, C.byref(p), C.c_void_p(stream)))
        del keep
        return self.thermal_download()

    # rate-coefficient tables from the cross-sections (include/artis_amd.h artis_amd_ratecoeff_*)
    def ratecoeff_tables(self, install: bool = False, items_per_launch: int = 0) -> dict:
        """artis_amd_ratecoeff_compute and the download: "spontrecombcoeffs", "bfcooling_coeffs" and (builds with USE_LUT_PHOTOION; else
        None) "corrphotoioncoeffs" as [nbfcontinua, TABLESIZE], "flags" alike (abi.RATECOEFF_*), and the counts of artis_ratecoeff_stats.
        install: copy the tables over the model's on the device (set-up phase only). A flagged entry raises; ratecoeff_download() still
        shows the tables and flags."""
        req = abi.RatecoeffRequest(struct_size=C.sizeof(abi.RatecoeffRequest), install=int(bool(install)), items_per_launch=int(items_per_launch))
        self._check(self.L.artis_amd_ratecoeff_compute(self.h, C.byref(req)))
        return self.ratecoeff_download()

    def ratecoeff_download(self) -> dict:
        stats = abi.RatecoeffStats(struct_size=C.sizeof(abi.RatecoeffStats))
        self._check(self.L.artis_amd_ratecoeff_download(self.h, None, None, None, None, C.byref(stats)))  # sizes first
        shape = (int(stats.nbfcontinua), int(stats.tablesize))
        n = max(shape[0] * shape[1], 1)
        spont, cool, flags = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
        gamma = np.zeros(n) if stats.ntables == 3 else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self.L.artis_amd_ratecoeff_download(self.h, ptr(spont), ptr(gamma), ptr(cool), ptr(flags), C.byref(stats)))
        cut = lambda a: None if a is None else a[: shape[0] * shape[1]].reshape(shape)
        out = dict(spontrecombcoeffs=cut(spont), corrphotoioncoeffs=cut(gamma), bfcooling_coeffs=cut(cool), flags=cut(flags))
        out.update({k: v for k, v in abi.struct_dict(stats).items() if k != "struct_size"})
        return out

    # photoionisation coefficients of builds without USE_LUT_PHOTOION (include/artis_amd.h artis_amd_set_cellstate_photoion)
    def set_cellstate_photoion(self, cells: abi.CellState, ts: abi.Timestep, use_bf_estimators: bool = False, bfrate_normed=None,
                               cells_per_launch: int = 0, stream: int = 0):
        """set_cellstate for a cell state without "corrphotoioncoeff": the engine computes it on the device from the state it uploads.
        use_bf_estimators: the host's timestep >= DETAILED_BF_ESTIMATORS_USEFROMTIMESTEP; bfrate_normed [ncell, nbfestim] float32, or
        None: the last radfield_fit's block, device to device. photoion() downloads what was computed."""
        bf = None if bfrate_normed is None else np.ascontiguousarray(bfrate_normed, dtype=np.float32).reshape(-1)
        p = abi.PhotoionParams(struct_size=C.sizeof(abi.PhotoionParams), use_bf_estimators=int(bool(use_bf_estimators)),
                               cells_per_launch=int(cells_per_launch))
        if bf is not None:
            p.bfrate_normed = bf.ctypes.data_as(C.POINTER(C.c_float))
        self._cells, self._ts = cells, ts
        self._check(self.L.artis_amd_set_cellstate_photoion(self.h, C.cast(cells.ref(), C.c_void_p), C.cast(ts.ref(), C.c_void_p), C.byref(p),
                                                            C.c_void_p(stream)))

    def photoion(self) -> dict:
        """artis_amd_photoion_download: "coeff" [ncell, nphixstargets_total], "source" alike (uint8, abi.PHOTOION_SRC_*), "flags" [ncell]
        (abi.PHOTOION_NONFINITE), "totals" as a dict over abi.PHOTOION_TOTALS, the sizes and "kernel_ms" """
        info = abi.PhotoionResult(struct_size=C.sizeof(abi.PhotoionResult))
        self._check(self.L.artis_amd_photoion_download(self.h, C.byref(info)))  # sizes first
        n, ne = info.npts_nonempty, info.nphixstargets_total
        out = dict(coeff=np.zeros(max(n * ne, 1)), source=np.zeros(max(n * ne, 1), np.uint8), flags=np.zeros(max(n, 1), np.int32))
        types = dict(abi.PhotoionResult._fields_)
        for k, v in out.items():
            setattr(info, k, v.ctypes.data_as(types[k]))
        self._check(self.L.artis_amd_photoion_download(self.h, C.byref(info)))
        out["coeff"] = out["coeff"][: n * ne].reshape(n, ne)
        out["source"] = out["source"][: n * ne].reshape(n, ne)
        out["flags"] = out["flags"][:n]
        out.update(totals={k: int(info.totals[i]) for i, k in enumerate(abi.PHOTOION_TOTALS)}, npts_nonempty=n, nphixstargets_total=ne,
                   nbfcontinua=int(info.nbfcontinua), nbfestim=int(info.nbfestim), kernel_ms=float(info.kernel_ms))
        return out

    def thermal_rates(self, bfheatingcoeffs, Te=None, rebalance: bool = False, ntlepton_dep=None, dep_alpha=None, dep_spfission=None,
                      stream: int = 0) -> dict:
        """The rates of every non-empty cell at Te (None: the resident T_e); rebalance False: with the resident n_e, populations,
        partition functions and matter; True: after the ion balance at Te with the last thermal_solve's Gamma. Returns the download."""
        p, keep = abi.thermal_params(bfheatingcoeffs, None, None, None, ntlepton_dep, dep_alpha, dep_spfission, None)
        te = None if Te is None else np.ascontiguousarray(Te, dtype=np.float32)
        self._check(self.L.artis_amd_thermal_rates(self.h, C.byref(p), te.ctypes.data_as(C.c_void_p) if te is not None else None,
                                                   int(bool(rebalance)), C.c_void_p(stream)))
        del keep
        return self.thermal_download()

    def thermal_download(self, arrays: bool = True) -> dict:
        """numpy arrays under the field names of artis_thermal_result (per-ion ones [ncell, nions], gamma and corrphotoionrenorm
        [ncell, nbfcontinua_ground], bracket [ncell, 2], rates [ncell, 10] in abi.THERMAL_RATES order), "ncells_flagged" as a dict over
        abi.THERMAL_FLAGS, "total_evals", "nfitted" and "kernel_ms" as a dict over abi.THERMAL_KERNELS; arrays=False: only those"""
        info = abi.ThermalResult(struct_size=C.sizeof(abi.ThermalResult))
        self._check(self.L.artis_amd_thermal_download(self.h, C.byref(info)))  # sizes first
        n, ni, g = info.npts_nonempty, info.nions, info.nbfcontinua_ground
        out = abi.thermal_arrays(n, ni, g) if arrays else {}
        types = dict(abi.ThermalResult._fields_)
        for k, v in out.items():
            setattr(info, k, v.ctypes.data_as(types[k]))
        if arrays:
            self._check(self.L.artis_amd_thermal_download(self.h, C.byref(info)))
            for k in ("ion_groundlevelpops", "ion_partfuncts", "phi"):
                out[k] = out[k].reshape(n, ni)
            for k in ("gamma", "corrphotoionrenorm"):
                out[k] = out[k][: n * g].reshape(n, g)
            out["bracket"] = out["bracket"].reshape(n, 2)
            out["rates"] = out["rates"].reshape(n, abi.THERMAL_NRATES)
        out["ncells_flagged"] = {k: int(info.ncells_flagged[i]) for i, k in enumerate(abi.THERMAL_FLAGS)}
        out.update(total_evals=int(info.total_evals), nfitted=int(info.nfitted),
                   kernel_ms={k: float(info.kernel_ms[i]) for i, k in enumerate(abi.THERMAL_KERNELS)})
        return out

    def grid_update_thermal(self, ts_next: abi.Timestep, thick=None, kappagrey=None, ffegrp=None, stream: int = 0) -> dict:
        """grid_update with the matter, the clumping factors, and in fitted cells the T_e, Gamma and corrphotoionrenorm of the last
        thermal_solve; thick None: the last deposition_update's flags. Returns the grid_update download."""
        u, keep = abi.grid_update_config(True, None, None, thick, None, None, None, None, None, kappagrey, None, ffegrp)
        self._check(self.L.artis_amd_grid_update_thermal(self.h, C.byref(u), C.cast(ts_next.ref(), C.c_void_p), C.c_void_p(stream)))
        self._ts = ts_next
        del keep
        return self.grid_update_download()

    def debug_cellcache(self, c: int) -> dict:
        d = self.model.d
        out = {
            "levelpops": np.zeros(d["nlevels"]), "maprocessrates": np.zeros(d["nlevels"] * 9),
            "matrans": np.zeros(max(d["nmatransblock"], 1)), "allcont_nnlevel": np.zeros(max(d["nbfcontinua"], 1)),
            "allcont_departure": np.zeros(max(d["nbfcontinua"], 1)), "allcont_edgepart": np.zeros(max(d["nbfcontinua"], 1)),
            "allcont_keepbits": np.zeros((d["nbfcontinua"] + 63) // 64 + 1, dtype=np.uint64),
            "corrphotoioncoeff": np.zeros(max(d["nphixstargets_total"], 1)),
            "cooling_contrib": np.zeros(max(d["ncoolingterms"], 1)), "ion_cooling_contribs": np.zeros(d["nions"]),
        }
        chi = C.c_double(0.0)
        args = [self.h, C.c_int(c)] + [v.ctypes.data_as(C.c_void_p) for v in out.values()] + [C.byref(chi)]
        self._check(self.L.artis_amd_debug_cellcache(*args))
        out["chi_ff_nnionpart"] = chi.value
        return out

    def debug_cellcache_array(self, c: int, which) -> np.ndarray:
        """artis_amd_debug_cellcache_array: one array of cell c's row as stored, typed (abi.CC_ARRAYS: name -> (enumerator, dtype, doubles per
        element); the two arrays of pairs come as (n, 2) float64). which: a name of abi.CC_ARRAYS or an enumerator. EngineError where the
        array does not exist in this build or model."""
        idx, dtype, width = abi.CC_ARRAYS[which] if isinstance(which, str) else next(v for v in abi.CC_ARRAYS.values() if v[0] == int(which))
        itemsize = np.dtype(dtype).itemsize
        need = C.c_int64(0)
        probe = np.zeros(1, dtype=np.uint8)
        self.L.artis_amd_debug_cellcache_array.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        rc = self.L.artis_amd_debug_cellcache_array(self.h, int(c), idx, probe.ctypes.data_as(C.c_void_p), 0, C.byref(need))  # (asks for the row's size)
        if need.value <= 0:
            self._check(rc)
            raise EngineError(f"artis_amd_debug_cellcache_array({which}): no size reported")
        assert need.value % (itemsize * width) == 0, (which, need.value)
        buf = np.zeros(need.value // itemsize, dtype=dtype)
        written = C.c_int64(0)
        self._check(self.L.artis_amd_debug_cellcache_array(self.h, int(c), idx, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(written)))
        assert written.value == buf.nbytes, (which, written.value, buf.nbytes)
        return buf.reshape(-1, 2) if width == 2 else buf

    def debug_sort_list(self, keys, lst, nkeys: int):
        """lst's entries ordered by non-decreasing key, by the many-keys work-list sort (artis_amd_debug_sort_list); keys[i] in [0, nkeys)
        is the key of lst[i]. The engine's own lists are not touched."""
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        lst = np.ascontiguousarray(lst, dtype=np.int32)
        assert keys.shape == lst.shape and keys.ndim == 1
        out = np.empty_like(lst)
        self.L.artis_amd_debug_sort_list.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]
        self._check(self.L.artis_amd_debug_sort_list(self.h, keys.ctypes.data_as(C.c_void_p), lst.ctypes.data_as(C.c_void_p), len(lst), int(nkeys),
                                                     out.ctypes.data_as(C.c_void_p)))
        return out

    def config(self) -> dict:
        """the configuration the engine runs with, every "automatic" resolved (artis_amd_engine_config): a dict over artis_amd_config's fields"""
        out = abi.config()
        self._check(self.L.artis_amd_engine_config(self.h, C.byref(out)))
        return abi.struct_dict(out)

    def cache_tiles(self):
        """(number of cell-cache tiles, cells per tile, cache bytes per cell)"""
        nt, cells, bpc = C.c_int32(), C.c_int64(), C.c_int64()
        self.L.artis_amd_cache_tiles.argtypes = [C.c_void_p] * 4
        self._check(self.L.artis_amd_cache_tiles(self.h, C.byref(nt), C.byref(cells), C.byref(bpc)))
        return nt.value, cells.value, bpc.value

    def record_tiers(self):
        """(share of every ion's levels with a static macro-atom record, cold levels, pool slots per resident cell): what the engine chose
        from its cache budget at creation, or was given (ARTIS_AMD_MA_HOTFRAC / _POOLFRAC)"""
        h, n, p = C.c_double(), C.c_int32(), C.c_int64()
        self.L.artis_amd_record_tiers.argtypes = [C.c_void_p] * 4
        self._check(self.L.artis_amd_record_tiers(self.h, C.byref(h), C.byref(n), C.byref(p)))
        return {"hot_fraction": h.value, "ncold": n.value, "pool_slots": p.value}

    THERMAL_PLAIN, THERMAL_LDS_TABLES, THERMAL_LDS_LEVELPACK, THERMAL_REFILL, THERMAL_COLD, THERMAL_TAIL = 1, 2, 4, 8, 16, 32
    THERMAL_LATE = 64

    def last_thermal_variants(self) -> int:
        """mask of the thermal-kernel forms the last step() launched (include/artis_amd.h ARTIS_AMD_THERMAL_*)"""
        m = C.c_int32()
        self.L.artis_amd_last_thermal_variants.argtypes = [C.c_void_p] * 2
        self._check(self.L.artis_amd_last_thermal_variants(self.h, C.byref(m)))
        return int(m.value)

    def last_estimator_forms(self) -> int:
        """mask of the ways the last step()'s kernels added to the per-cell estimators (abi.EST_FORMS, include/artis_amd.h ARTIS_AMD_EST_*)"""
        m = C.c_int32()
        self.L.artis_amd_last_estimator_forms.argtypes = [C.c_void_p] * 2
        self._check(self.L.artis_amd_last_estimator_forms(self.h, C.byref(m)))
        return int(m.value)

    def last_tiling(self):
        """sweeps over the cache tiles, tile fills, their summed ms and the packets listed in the last step()"""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_double(), C.c_int64()
        self.L.artis_amd_last_tiling.argtypes = [C.c_void_p] * 5
        self._check(self.L.artis_amd_last_tiling(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        e, f = C.c_int64(), C.c_int64()
        self.L.artis_amd_last_tiling_fills.argtypes = [C.c_void_p] * 3
        self._check(self.L.artis_amd_last_tiling_fills(self.h, C.byref(e), C.byref(f)))
        g = C.c_int64()
        self.L.artis_amd_last_tiling_parked.argtypes = [C.c_void_p] * 2
        self._check(self.L.artis_amd_last_tiling_parked(self.h, C.byref(g)))
        r = C.c_int64()
        self.L.artis_amd_last_pool_resets.argtypes = [C.c_void_p] * 2
        self._check(self.L.artis_amd_last_pool_resets(self.h, C.byref(r)))
        pu, pc = C.c_int64(), C.c_int64()
        self.L.artis_amd_last_pool_usage.argtypes = [C.c_void_p] * 3
        self._check(self.L.artis_amd_last_pool_usage(self.h, C.byref(pu), C.byref(pc)))
        return {"sweeps": a.value, "tile_fills": b.value, "fill_ms": c.value, "listed": d.value, "sparse_fills": e.value,
                "cells_filled": f.value, "parked": g.value, "pool_resets": r.value, "pool_units_used": pu.value, "pool_units": pc.value}

    def last_absent_records(self):
        """(static macro-atom records of absent ions the last cell-cache population left out, records the last step() filled on demand)"""
        a, b = C.c_int64(), C.c_int64()
        self.L.artis_amd_last_absent_records.argtypes = [C.c_void_p] * 3
        self._check(self.L.artis_amd_last_absent_records(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # estimator reduction in the C++ host layer (RCCL)
    COMM_ID_BYTES = 128

    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(self.COMM_ID_BYTES)
        self.L.artis_amd_comm_unique_id.argtypes = [C.c_void_p]
        self._check(self.L.artis_amd_comm_unique_id(buf))
        return buf.raw

    def comm_count(self) -> int:
        """ranks of the engine's communicator as RCCL reports them (ncclCommCount)"""
        n = C.c_int(0)
        self.L.artis_amd_comm_count.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        self._check(self.L.artis_amd_comm_count(self.h, None, C.byref(n)))
        return int(n.value)

    def comm_init(self, nranks: int, rank: int, id_bytes: bytes):
        assert len(id_bytes) == self.COMM_ID_BYTES
        self.L.artis_amd_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
        self._check(self.L.artis_amd_comm_init(self.h, nranks, rank, id_bytes))

    def allreduce_estimators(self, stream: int = 0, comm: int = 0):
        self.L.artis_amd_allreduce_estimators.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.L.artis_amd_allreduce_estimators(self.h, C.c_void_p(comm), C.c_void_p(stream)))

    def last_kernel_breakdown(self):
        a, b, c, d = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        self.L.artis_amd_last_kernel_breakdown.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        self._check(self.L.artis_amd_last_kernel_breakdown(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        e, f = C.c_int64(), C.c_int64()
        self.L.artis_amd_last_kernel_launches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.L.artis_amd_last_kernel_launches(self.h, C.byref(e), C.byref(f)))
        return {"rpkt_ms": a.value, "rpkt_threads": b.value, "rpkt_launches": e.value, "thermal_ms": c.value,
                "thermal_threads": d.value, "thermal_launches": f.value}

    def last_kernel_table(self):
        ms, nl, npk = (C.c_double * 4)(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
        self.L.artis_amd_last_kernel_table.argtypes = [C.c_void_p] * 4
        self._check(self.L.artis_amd_last_kernel_table(self.h, ms, nl, npk))
        names = ["k_rpkt", "k_ma", "k_kpkt", "k_slow"]
        return {n: {"ms": ms[i], "launches": nl[i], "packets": npk[i]} for i, n in enumerate(names)}

    def last_kernel_ms_by_kind(self):
        ms, nl = (C.c_double * 8)(), (C.c_int64 * 8)()
        self.L.artis_amd_last_kernel_ms_by_kind.argtypes = [C.c_void_p] * 3
        self._check(self.L.artis_amd_last_kernel_ms_by_kind(self.h, ms, nl))
        names = ["k_rpkt", "k_thermal", "k_slow", "k_gamma", "k_blackbody", "k_tail", "tile_fills", "k_late"]
        return {n: {"ms": round(ms[i], 3), "launches": nl[i]} for i, n in enumerate(names)}

    def last_kernel_ms(self):
        ms, n = C.c_double(), C.c_int64()
        self._check(self.L.artis_amd_last_kernel_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value
