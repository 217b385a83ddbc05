"""ctypes mirror of include/artis_amd.h (the C-ABI structs), backed by numpy arrays.

This is plumbing for tests and bench.py: it only describes memory that is handed
to the C-ABI (the HIP engine, or -- from tests -- the CPU oracle). It contains no
physics.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

STAT_X_VPKT_CREATED = 48  # then _ESC_RPKT, _ESC_KPKT, _ESC_MA (include/artis_amd.h ARTIS_STAT_X_VPKT_*)
ABI_VERSION = 6  # artis_amd_abi_version() of the library these ctypes structs describe (include/artis_amd.h)
NSTATS = 64
NSCALARS = 11  # ARTIS_SCALAR_* of include/artis_amd.h
SCALAR_NAMES = ["gamma_dep_discrete", "nt_energy_deposited", "pellet_decays", "gamma_emission", "positron_emission",
                "electron_emission", "alpha_emission", "spfission_dep_discrete", "electron_dep_discrete",
                "positron_dep_discrete", "alpha_dep_discrete"]
# artis_amd_last_estimator_forms(): how the kernels of the last call added to the per-cell estimators (include/artis_amd.h ARTIS_AMD_EST_*)
EST_FORMS = {"RPKT_LDS_CONT": 1, "RPKT_LDS_NOCONT": 2, "RPKT_LDS_LINE": 32768, "RPKT_WAVECACHE": 4, "RPKT_GLOBAL": 8,
             "THERMAL_LDS": 16, "THERMAL_WAVECACHE": 32, "THERMAL_GLOBAL": 64, "GAMMA_LDS": 128, "GAMMA_GLOBAL": 256,
             "BF_INPLACE": 512, "BF_DENSE_CONTLDS": 1024, "BF_DENSE_HBM": 2048, "BF_LPR16": 4096, "BF_LPR32": 8192, "BF_LPR64": 16384}


def est_form_names(mask: int) -> list:
    return [k for k, v in EST_FORMS.items() if mask & v]


STAT_COUNT = 34
STAT_X_RPKT_STEPS = 34
STAT_X_KPKT_STEPS = 35
STAT_X_LINES_VISITED = 36
STAT_X_MA_JUMPS = 37
STAT_X_GAMMA_STEPS = 40

TYPE_GAMMA = 10
TYPE_RPKT = 11
TYPE_KPKT = 12
TYPE_NTLEPTON_DEPOSITED = 20
TYPE_NONTHERMAL_PREDEPOSIT_BETAMINUS = 21
TYPE_NONTHERMAL_PREDEPOSIT_BETAPLUS = 22
TYPE_NONTHERMAL_PREDEPOSIT_ALPHA = 23
TYPE_NTALPHA_FISPROD_DEPOSITED = 24
TYPE_RADIOACTIVE_PELLET = 100
TYPE_ESCAPE = 32
TYPE_PRE_KPKT = 120
EMTYPE_NOTSET = -9999000
EMTYPE_FREEFREE = -9999999

GRID_SPHERICAL1D = 0
GRID_CYLINDRICAL2D = 1
GRID_CARTESIAN3D = 2

STAT_NAMES = [
    "MA_STAT_ACTIVATION_COLLEXC", "MA_STAT_ACTIVATION_COLLION", "MA_STAT_ACTIVATION_NTCOLLEXC",
    "MA_STAT_ACTIVATION_NTCOLLION", "MA_STAT_ACTIVATION_BB", "MA_STAT_ACTIVATION_BF", "MA_STAT_ACTIVATION_FB",
    "MA_STAT_DEACTIVATION_COLLDEEXC", "MA_STAT_DEACTIVATION_COLLRECOMB", "MA_STAT_DEACTIVATION_BB",
    "MA_STAT_DEACTIVATION_FB", "MA_STAT_INTERNALUPHIGHER", "MA_STAT_INTERNALUPHIGHERNT",
    "MA_STAT_INTERNALDOWNLOWER", "K_STAT_TO_MA_COLLEXC", "K_STAT_TO_MA_COLLION", "K_STAT_TO_R_FF", "K_STAT_TO_R_FB",
    "K_STAT_TO_R_BB", "K_STAT_FROM_FF", "K_STAT_FROM_BF", "NT_STAT_FROM_GAMMA", "NT_STAT_TO_IONISATION",
    "NT_STAT_TO_EXCITATION", "NT_STAT_TO_KPKT", "K_STAT_FROM_EARLIERDECAY", "INTERACTIONS", "ELECTRON_SCATTERINGS",
    "RESONANCESCATTERINGS", "CELLCROSSINGS", "UPSCATTER", "DOWNSCATTER", "UPDATECELL", "PKTESCAPES",
    "X_RPKT_STEPS", "X_KPKT_STEPS", "X_LINES_VISITED", "X_MA_JUMPS", "X_CHI_EVALS", "X_CONT_VISITED",
    "X_GAMMA_STEPS",
] + [f"X_{i}" for i in range(41, 64)]

# struct artis_packet (include/artis_amd.h), natural C alignment == numpy align=True
PACKET_DTYPE = np.dtype(
    [
        ("rngstate", np.uint32, (4,)),
        ("prop_time", np.float64),
        ("pos", np.float64, (3,)),
        ("dir", np.float64, (3,)),
        ("nu_cmf", np.float64),
        ("e_cmf", np.float64),
        ("nu_rf", np.float64),
        ("e_rf", np.float64),
        ("next_trans", np.int32),
        ("nscatterings", np.int32),
        ("emissiontype", np.int32),
        ("em_pos", np.float64, (3,)),
        ("em_time", np.float32),
        ("absorptiontype", np.int32),
        ("absorptionfreq", np.float64),
        ("stokes_q", np.float64),
        ("stokes_u", np.float64),
        ("trueemissiontype", np.int32),
        ("trueem_pos", np.float64, (3,)),
        ("trueem_time", np.float32),
        ("type", np.int32),
        ("cellindex", np.int32),
        ("escape_type", np.int32),
        ("escape_time", np.float32),
        ("tdecay", np.float64),
        ("number", np.int32),
        ("originated_from_particlenotgamma", np.uint8),
        ("pellet_decaytype", np.int32),
        ("pellet_nucindex", np.int32),
    ],
    align=True,
)

PACKET_INT_FIELDS = ["next_trans", "nscatterings", "emissiontype", "absorptiontype", "trueemissiontype", "type",
                     "cellindex", "escape_type", "number"]
PACKET_FLOAT_FIELDS = ["prop_time", "pos", "dir", "nu_cmf", "e_cmf", "nu_rf", "e_rf", "em_pos", "em_time",
                       "absorptionfreq", "stokes_q", "stokes_u", "trueem_pos", "trueem_time", "escape_time"]

_I32P = C.POINTER(C.c_int32)
_F32P = C.POINTER(C.c_float)
_F64P = C.POINTER(C.c_double)
_U8P = C.POINTER(C.c_uint8)
_I64P = C.POINTER(C.c_int64)

# (name, ctype-or-pointer, numpy dtype or None for scalars) in the exact order of struct artis_model
_MODEL_FIELDS = [
    ("nelements", C.c_int32, None), ("nions", C.c_int32, None), ("nlevels", C.c_int32, None),
    ("nlines", C.c_int32, None), ("nalltrans", C.c_int32, None), ("nphixstargets_total", C.c_int32, None),
    ("nphixslevels", C.c_int32, None), ("nbfcontinua", C.c_int32, None), ("nbfcontinua_ground", C.c_int32, None),
    ("ncoolingterms", C.c_int32, None), ("nmatransblock", C.c_int32, None), ("NPHIXSPOINTS", C.c_int32, None),
    ("NPHIXSNUINCREMENT", C.c_double, None),
    ("elem_nions", _I32P, np.int32), ("elem_uniqueionindexstart", _I32P, np.int32), ("elem_anumber", _I32P, np.int32),
    ("elem_lowest_ionstage", _I32P, np.int32),
    ("ion_element", _I32P, np.int32), ("ion_nlevels", _I32P, np.int32), ("ion_nlevels_ionising", _I32P, np.int32),
    ("ion_maxrecombininglevel", _I32P, np.int32), ("ion_uniquelevelindexstart", _I32P, np.int32),
    ("ion_coolingoffset", _I32P, np.int32), ("ion_ncoolingterms", _I32P, np.int32),
    ("level_epsilon", _F64P, np.float64), ("level_statweight", _F32P, np.float32),
    ("level_alltrans_startdown", _I32P, np.int32), ("level_ndowntrans", _I32P, np.int32),
    ("level_nuptrans", _I32P, np.int32), ("level_closestgroundlevelcont", _I32P, np.int32),
    ("level_phixsstart", _I32P, np.int32), ("level_nphixstargets", _I32P, np.int32),
    ("level_phixstargetstart", _I32P, np.int32), ("level_bflist_start", _I32P, np.int32),
    ("level_matransblock_start", _I32P, np.int32),
    ("alltrans_lineindex", _I32P, np.int32), ("alltrans_targetlevelindex", _I32P, np.int32),
    ("alltrans_einstein_A", _F32P, np.float32), ("alltrans_coll_str", _F32P, np.float32),
    ("alltrans_osc_strength", _F32P, np.float32), ("alltrans_forbidden", _U8P, np.uint8),
    ("line_nu", _F64P, np.float64), ("line_elementindex", _I32P, np.int32), ("line_ionindex", _I32P, np.int32),
    ("line_uniquelevelindex_lower", _I32P, np.int32), ("line_uniquelevelindex_upper", _I32P, np.int32),
    ("line_B_ul", _F32P, np.float32), ("line_B_lu", _F32P, np.float32),
    ("allphixs", _F32P, np.float32), ("allphixstargets_levelindex", _I32P, np.int32),
    ("allphixstargets_probability", _F64P, np.float64),
    ("allcont_nu_edge", _F64P, np.float64), ("allcont_element", _I32P, np.int32), ("allcont_ion", _I32P, np.int32),
    ("allcont_level", _I32P, np.int32), ("allcont_phixstargetindex", _I32P, np.int32),
    ("allcont_upperlevel", _I32P, np.int32), ("allcont_uniquelevelindex", _I32P, np.int32),
    ("allcont_probability", _F64P, np.float64), ("allcont_groundcontestimindex", _I32P, np.int32),
    ("groundcont_nu_edge", _F64P, np.float64),
    ("spontrecombcoeffs", _F64P, np.float64), ("corrphotoioncoeffs", _F64P, np.float64),
    ("bfcooling_coeffs", _F64P, np.float64),
    ("coolinglist_type", _U8P, np.uint8), ("coolinglist_level", _I32P, np.int32),
    ("coolinglist_phixstargetindex", _I32P, np.int32),
    ("gridtype", C.c_int32, None), ("ncoordgrid", C.c_int32 * 3, "i3"), ("ngrid", C.c_int32, None),
    ("npts_nonempty", C.c_int32, None), ("tmin", C.c_double, None), ("vmax", C.c_double, None),
    ("rmax", C.c_double, None), ("coord_pos_min_tmin", _F64P * 3, "p3"), ("propcell_nonemptymgi", _I32P, np.int32),
    # optional (NULL when absent): static inputs of the non-thermal channels
    ("elem_meannucmass", _F32P, np.float32), ("ion_nt_sum_q_over_binding", _F64P, np.float64),
    ("ejecta_kinetic_energy", C.c_double, None), ("mtot_input", C.c_double, None),
    ("allcont_bfestimindex", _I32P, np.int32), ("nbfestim", C.c_int32, None),
    ("rho_tmin", _F32P, np.float32),
    ("xcom_elem_start", _I32P, np.int32), ("xcom_energy", _F64P, np.float64), ("xcom_sigma", _F64P, np.float64),
    ("detailed_lineindices", _I32P, np.int32), ("detailed_linecount", C.c_int32, None),
    # optional: the virtual-packet configuration (vpkt.txt as read_vpktparameterfile() leaves it; builds with VPKT_ON)
    ("vpkt_nobsdirections", C.c_int32, None), ("vpkt_obsdirs_costheta", _F64P, np.float64), ("vpkt_obsdirs_phi", _F64P, np.float64),
    ("vpkt_nspectraperobsdir", C.c_int32, None), ("vpkt_opacityexclusions", _I32P, np.int32),
    ("vpkt_timemin_input", C.c_double, None), ("vpkt_timemax_input", C.c_double, None),
    ("vpkt_nwavelengthranges", C.c_int32, None), ("vpkt_numin_input", _F64P, np.float64), ("vpkt_numax_input", _F64P, np.float64),
    ("vpkt_tau_max", C.c_double, None), ("vpkt_vgrid_on", C.c_int32, None),
    ("vpkt_tmin_grid", C.c_double, None), ("vpkt_tmax_grid", C.c_double, None),
    ("vpkt_grid_nwavelengthranges", C.c_int32, None), ("vpkt_nu_grid_min", _F64P, np.float64), ("vpkt_nu_grid_max", _F64P, np.float64),
    ("vpkt_nprocs", C.c_int32, None),
]
VSPEC_NUBINS, VSPEC_TIMEBINS, VGRID_NY, VGRID_NZ = 2500, 5, 50, 50  # vpkt.h:21-32
_MODEL_OPTIONAL = ("elem_meannucmass", "ion_nt_sum_q_over_binding", "ejecta_kinetic_energy", "mtot_input",
                   "allcont_bfestimindex", "nbfestim", "rho_tmin", "xcom_elem_start", "xcom_energy", "xcom_sigma",
                   "detailed_lineindices", "detailed_linecount",
                   "vpkt_nobsdirections", "vpkt_obsdirs_costheta", "vpkt_obsdirs_phi", "vpkt_nspectraperobsdir",
                   "vpkt_opacityexclusions", "vpkt_timemin_input", "vpkt_timemax_input", "vpkt_nwavelengthranges",
                   "vpkt_numin_input", "vpkt_numax_input", "vpkt_tau_max", "vpkt_vgrid_on", "vpkt_tmin_grid", "vpkt_tmax_grid",
                   "vpkt_grid_nwavelengthranges", "vpkt_nu_grid_min", "vpkt_nu_grid_max", "vpkt_nprocs")

_CELL_FIELDS = [
    ("rho", _F32P, np.float32), ("Te", _F32P, np.float32), ("TJ", _F32P, np.float32), ("TR", _F32P, np.float32),
    ("W", _F32P, np.float32), ("nne", _F32P, np.float32), ("nnetot", _F32P, np.float32),
    ("kappagrey", _F32P, np.float32), ("thick", _I32P, np.int32), ("clumpfactor", _F32P, np.float32),
    ("ion_groundlevelpops", _F32P, np.float32), ("ion_partfuncts", _F32P, np.float32),
    ("elem_massfracs", _F32P, np.float32), ("corrphotoionrenorm", _F64P, np.float64),
    ("ffegrp", _F32P, np.float32),
    # optional (NULL when absent from the dict): host level populations, host photoionisation coefficients, multibin field
    ("levelpops", _F64P, np.float64), ("corrphotoioncoeff", _F64P, np.float64),
    ("radfieldbin_W", _F32P, np.float32), ("radfieldbin_T_R", _F32P, np.float32),
    # optional: the Spencer-Fano solution (builds with NT_ON)
    ("nt_frac_ionisation", _F32P, np.float32), ("nt_frac_excitation", _F32P, np.float32),
    ("nt_deposition_rate_density", _F64P, np.float64), ("nt_eff_ionpot", _F32P, np.float32),
    ("nt_prob_num_auger", _F32P, np.float32), ("nt_ionenfrac_num_auger", _F32P, np.float32),
    ("nt_exc_count", _I32P, np.int32), ("nt_exc_frac_deposition", _F64P, np.float64),
    ("nt_exc_ratecoeffperdeposition", _F64P, np.float64), ("nt_exc_alltransindex", _I32P, np.int32),
    ("nt_excitations_stored", C.c_int32, None),
    ("expansionopacities", _F32P, np.float32), ("expansionopacity_planck_cumulative", _F64P, np.float64),
    ("Jb_lu_normed", _F64P, np.float64),
    ("elem_meanweight", _F32P, np.float32),
]
EXPOPAC_NBINS = 1997
_CELL_OPTIONAL = ("levelpops", "corrphotoioncoeff", "radfieldbin_W", "radfieldbin_T_R", "nt_frac_ionisation",
                  "nt_frac_excitation", "nt_deposition_rate_density", "nt_eff_ionpot", "nt_prob_num_auger",
                  "nt_ionenfrac_num_auger", "nt_exc_count", "nt_exc_frac_deposition", "nt_exc_ratecoeffperdeposition",
                  "nt_exc_alltransindex", "nt_excitations_stored", "expansionopacities", "expansionopacity_planck_cumulative", "Jb_lu_normed",
                  "elem_meanweight")
# enum artis_amd_cc_array of include/artis_amd.h (artis_amd_debug_cellcache_array): name -> (enumerator, element type, elements per entry)
CC_ARRAYS = {
    "line_dpop": (0, np.float64, 1), "bf_radrecomb": (1, np.float64, 1), "bf_colrecomb": (2, np.float64, 1), "bf_colion": (3, np.float64, 1),
    "bf_cooling": (4, np.float64, 1), "allcont_pair": (5, np.float64, 2), "allcont_keptlist": (6, np.int32, 1),
    "allcont_keepprefix": (7, np.int32, 1), "allcont_keptpair": (8, np.float64, 2), "cool_guide": (9, np.uint16, 1),
    "ion_cooling_C": (10, np.float64, 1), "expansionopacities": (11, np.float32, 1),
    "expansionopacity_planck_cumulative": (12, np.float64, 1), "nt_ionratecoeff": (13, np.float64, 1), "nt_ionenrate_cum": (14, np.float64, 1),
    "allcont_keepbits": (15, np.uint64, 1),
}
NT_NAUGER = 3  # NT_MAX_AUGER_ELECTRONS + 1
RADFIELDBINCOUNT = 256
# options presets with the multibin radiation field and the detailed bound-free estimators (artisoptions_nltenebular.h and
# the three files that differ from it in constants): RADFIELDBINCOUNT of each
NEBULAR_FAMILY = {"nltenebular": 256, "christinenonthermal": 64, "nltephotospheric": 256, "nltewithoutnonthermal": 512,
                  "nltenebular_lineest": 256, "ci_nebular": 256, "ci_nebular_limitbfest": 256, "ci_nltephotospheric": 24}
# The option sets of the reference's CI (tests/setup_*.sh; include/artis_options.h ARTIS_PRESET_CI_*): the setup script, the
# preset whose host inputs the build needs (what synth.build hands over), and TABLESIZE / MINTEMP / MAXTEMP
CI_PRESETS = {
    "ci_kilonova": ("setup_kilonova_2d.sh", "kilonova_lte", (20, 1000.0, 20000.0)),
    "ci_kilonova_barnes": ("setup_kilonova_2d_barnesthermalisation.sh", "kilonova_lte", (20, 1000.0, 20000.0)),
    "ci_kilonova_expopac": ("setup_kilonova_2d_expansionopac.sh", "kilonova_expopac", (20, 1000.0, 20000.0)),
    "ci_kilonova_xcom": ("setup_kilonova_2d_xcomgammaphotoion.sh", "classic_gamma_xcom", (20, 1000.0, 20000.0)),
    "ci_nebular": ("setup_nebular_1d_3dgrid.sh", "nltenebular", (20, 2000.0, 10000.0)),
    "ci_nebular_limitbfest": ("setup_nebular_1d_3dgrid_limitbfest.sh", "nltephotospheric", (20, 2000.0, 10000.0)),
    "ci_nltephotospheric": ("setup_nltephotospheric_dynamic_ion_range_1d_1dgrid.sh", "nltephotospheric", (40, 3500.0, 140000.0)),
    # classic + virtual packets (VPKT_ON): line by line, and with the binned expansion opacities beyond the first bin
    "ci_classic_vpkt": ("setup_classicmode_1d_3dgrid.sh", "classic", (100, 3500.0, 140000.0)),
    "ci_classic_vpkt_expopac": ("setup_classicmode_3d.sh", "classic", (100, 3500.0, 140000.0)),
}


def inputs_like(options: str) -> str:
    """the preset whose kind of host inputs (synth.build) an options preset needs"""
    return CI_PRESETS[options][1] if options in CI_PRESETS else options


class CModel(C.Structure):
    _fields_ = [(n, t) for n, t, _ in _MODEL_FIELDS]


class CCellState(C.Structure):
    _fields_ = [(n, t) for n, t, _ in _CELL_FIELDS]


class CTimestep(C.Structure):
    _fields_ = [("nts", C.c_int32), ("start", C.c_double), ("width", C.c_double), ("mid", C.c_double),
                ("max_path_step", C.c_double)]


class CEstimators(C.Structure):
    _fields_ = [("J", _F64P), ("nuJ", _F64P), ("ffheatingestimator", _F64P), ("colheatingestimator", _F64P),
                ("gammaestimator", _F64P), ("bfheatingestimator", _F64P), ("stats", _I64P),
                ("dep_estimator_gamma", _F64P), ("scalars", _F64P), ("dep_estimator_electron", _F64P),
                ("dep_estimator_positron", _F64P), ("dep_estimator_alpha", _F64P),
                ("radfieldbin_J", _F64P), ("radfieldbin_nuJ", _F64P), ("bfrate_raw", _F64P),
                ("Jb_lu_raw", _F64P), ("Jb_lu_contribcount", _I64P), ("vspecpol", _F64P), ("vgrid_flux", _F64P)]


def _as_ptr(arr: np.ndarray, ptype):
    return arr.ctypes.data_as(ptype)


class Model:
    """Static model: dict of numpy arrays + scalars -> struct artis_model."""

    def __init__(self, d: dict):
        self.d = {}
        self.c = CModel()
        for name, ctype, npdt in _MODEL_FIELDS:
            if name in _MODEL_OPTIONAL and d.get(name) is None:
                continue  # stays a NULL pointer
            v = d[name]
            if npdt is None:
                setattr(self.c, name, v)
                self.d[name] = v
            elif npdt == "i3":
                arr = np.ascontiguousarray(v, dtype=np.int32)
                self.d[name] = arr
                for k in range(3):
                    self.c.ncoordgrid[k] = int(arr[k])
            elif npdt == "p3":
                arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in v]
                self.d[name] = arrs
                for k in range(3):
                    self.c.coord_pos_min_tmin[k] = _as_ptr(arrs[k], _F64P)
            else:
                arr = np.ascontiguousarray(v, dtype=npdt)
                if arr.size == 0:  # keep a valid pointer for empty tables
                    arr = np.zeros(1, dtype=npdt)
                self.d[name] = arr
                setattr(self.c, name, _as_ptr(arr, ctype))

    def __getitem__(self, k):
        return self.d[k]

    def ref(self):
        return C.byref(self.c)


class CellState:
    def __init__(self, d: dict):
        self.d = {}
        self.c = CCellState()
        for name, ctype, npdt in _CELL_FIELDS:
            if name in _CELL_OPTIONAL and d.get(name) is None:
                continue  # stays a NULL pointer
            if npdt is None:
                setattr(self.c, name, int(d[name]))
                self.d[name] = int(d[name])
                continue
            arr = np.ascontiguousarray(d[name], dtype=npdt)
            if arr.size == 0:
                arr = np.zeros(1, dtype=npdt)
            self.d[name] = arr
            setattr(self.c, name, _as_ptr(arr, ctype))

    def __getitem__(self, k):
        return self.d[k]

    def ref(self):
        return C.byref(self.c)


class Timestep:
    def __init__(self, nts: int, start: float, width: float, mid: float, max_path_step: float):
        self.c = CTimestep(nts, start, width, mid, max_path_step)

    def ref(self):
        return C.byref(self.c)


class Estimators:
    """Host estimator arrays (accumulated into by update_packets)."""

    def __init__(self, npts_nonempty: int, nbfcontinua_ground: int, nbfcontinua: int = 0, nbins: int = RADFIELDBINCOUNT,
                 ndetailedlines: int = 0, vpkt_shape=None):
        """vpkt_shape = (nobsdirections * nspectraperobsdir, nobsdirections * grid_nwavelengthranges or 0): also the
        virtual-packet spectra and velocity-grid map (builds with VPKT_ON). nbfcontinua > 0: also the estimators of the nltenebular options (radiation-field bins, detailed bound-free;
        nbfcontinua = the number of bound-free estimators, nbins = RADFIELDBINCOUNT of the options preset)"""
        n, g = npts_nonempty, max(nbfcontinua_ground, 1)
        self.radfieldbin_J = np.zeros(n * nbins if nbfcontinua > 0 else 1)
        self.radfieldbin_nuJ = np.zeros(n * nbins if nbfcontinua > 0 else 1)
        self.bfrate_raw = np.zeros(n * nbfcontinua if nbfcontinua > 0 else 1)
        self.Jb_lu_raw = np.zeros(max(n * ndetailedlines, 1))
        self.Jb_lu_contribcount = np.zeros(max(n * ndetailedlines, 1), dtype=np.int64)
        self.lineest = ndetailedlines > 0
        self.extended = nbfcontinua > 0
        self.vpkt = vpkt_shape is not None
        ncomb, ngridcomb = vpkt_shape if self.vpkt else (0, 0)
        self.vspecpol = np.zeros(max(VSPEC_TIMEBINS * ncomb * VSPEC_NUBINS * 3, 1))
        self.vgrid_flux = np.zeros(max(VGRID_NY * VGRID_NZ * ngridcomb * 3, 1))
        self.J = np.zeros(n)
        self.nuJ = np.zeros(n)
        self.ffheatingestimator = np.zeros(n)
        self.colheatingestimator = np.zeros(n)
        self.gammaestimator = np.zeros(n * g)
        self.bfheatingestimator = np.zeros(n * g)
        self.stats = np.zeros(NSTATS, dtype=np.int64)
        self.dep_estimator_gamma = np.zeros(n)
        self.scalars = np.zeros(NSCALARS)
        self.dep_estimator_electron = np.zeros(n)
        self.dep_estimator_positron = np.zeros(n)
        self.dep_estimator_alpha = np.zeros(n)
        self.c = CEstimators(
            _as_ptr(self.J, _F64P), _as_ptr(self.nuJ, _F64P), _as_ptr(self.ffheatingestimator, _F64P),
            _as_ptr(self.colheatingestimator, _F64P), _as_ptr(self.gammaestimator, _F64P),
            _as_ptr(self.bfheatingestimator, _F64P), _as_ptr(self.stats, _I64P),
            _as_ptr(self.dep_estimator_gamma, _F64P), _as_ptr(self.scalars, _F64P),
            _as_ptr(self.dep_estimator_electron, _F64P), _as_ptr(self.dep_estimator_positron, _F64P),
            _as_ptr(self.dep_estimator_alpha, _F64P),
            _as_ptr(self.radfieldbin_J, _F64P) if self.extended else None,
            _as_ptr(self.radfieldbin_nuJ, _F64P) if self.extended else None,
            _as_ptr(self.bfrate_raw, _F64P) if self.extended else None,
            _as_ptr(self.Jb_lu_raw, _F64P) if self.lineest else None,
            _as_ptr(self.Jb_lu_contribcount, _I64P) if self.lineest else None,
            _as_ptr(self.vspecpol, _F64P) if self.vpkt else None,
            _as_ptr(self.vgrid_flux, _F64P) if (self.vpkt and ngridcomb > 0) else None)

    def ref(self):
        return C.byref(self.c)

    def arrays(self):
        ext = {"radfieldbin_J": self.radfieldbin_J, "radfieldbin_nuJ": self.radfieldbin_nuJ,
               "bfrate_raw": self.bfrate_raw} if self.extended else {}
        if self.lineest:
            ext = {**ext, "Jb_lu_raw": self.Jb_lu_raw, "Jb_lu_contribcount": self.Jb_lu_contribcount}
        if self.vpkt:
            ext = {**ext, "vspecpol": self.vspecpol, "vgrid_flux": self.vgrid_flux}
        return {**ext, "J": self.J, "nuJ": self.nuJ, "ffheatingestimator": self.ffheatingestimator,
                "colheatingestimator": self.colheatingestimator, "gammaestimator": self.gammaestimator,
                "bfheatingestimator": self.bfheatingestimator, "dep_estimator_gamma": self.dep_estimator_gamma,
                "scalars": self.scalars, "dep_estimator_electron": self.dep_estimator_electron,
                "dep_estimator_positron": self.dep_estimator_positron, "dep_estimator_alpha": self.dep_estimator_alpha}

    def stats_dict(self):
        return {STAT_NAMES[i]: int(self.stats[i]) for i in range(NSTATS)}


def estimators_for(model, options: str = "classic") -> Estimators:
    """Estimator arrays sized for a model under an options preset (nltenebular adds the bin and bound-free arrays)"""
    if "vpkt" in options:
        nobs = model.d.get("vpkt_nobsdirections") or 0
        ngrid = (model.d.get("vpkt_grid_nwavelengthranges") or 0) if model.d.get("vpkt_vgrid_on") else 0
        return Estimators(model["npts_nonempty"], model["nbfcontinua_ground"],
                          vpkt_shape=(nobs * (model.d.get("vpkt_nspectraperobsdir") or 0), nobs * ngrid))
    if options not in NEBULAR_FAMILY:
        return Estimators(model["npts_nonempty"], model["nbfcontinua_ground"])
    nest = model.d.get("nbfestim") or model["nbfcontinua"]
    nlines = (model.d.get("detailed_linecount") or 0) if options.endswith("_lineest") else 0  # (no CI option set has them)
    return Estimators(model["npts_nonempty"], model["nbfcontinua_ground"], nest, NEBULAR_FAMILY[options], nlines)


def packets_ptr(packets: np.ndarray):
    assert packets.dtype == PACKET_DTYPE and packets.flags["C_CONTIGUOUS"]
    return packets.ctypes.data_as(C.c_void_p)


def seed_packet_rng(packets: np.ndarray, seed_base: int) -> None:
    """Per-packet Xoshiro128PP seeding: seed = seed_base + n through SplitMix32
    (reference random.h:32-40, 78-93, 117-123 and input.cc:1912-1916)."""
    n = len(packets)
    seed = (np.uint64(seed_base) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        st = seed + np.uint64(0x9E3779B97F4A7C15)
        st = (st ^ (st >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        st = (st ^ (st >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        sm = ((st ^ (st >> np.uint64(31))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        out = np.empty((n, 4), dtype=np.uint32)
        for i in range(4):
            sm = sm + np.uint32(0x9E3779B9)
            r = sm.copy()
            r = (r ^ (r >> np.uint32(16))) * np.uint32(0x21F0AAAD)
            r = (r ^ (r >> np.uint32(15))) * np.uint32(0x735A2D97)
            out[:, i] = r ^ (r >> np.uint32(15))
    packets["rngstate"] = out


# ---- emergent spectra and light curves (include/artis_amd.h artis_spectra_config / artis_spectra)
SPEC_MNUBINS = 1000
SPEC_MABINS = 100
SPEC_ALL_DIRBINS = -2
SPEC_OUTPUTS = ["lum", "lumcmf", "flux", "flux_q", "flux_u", "emission", "emission_q", "emission_u", "trueemission", "absorption",
                "absorption_q", "absorption_u", "gamma_lum", "gamma_lumcmf", "gamma_flux"]


class SpectraConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("ntimesteps", C.c_int32), ("dirbin", C.c_int32), ("ts_start", _F64P),
                ("ts_width", _F64P), ("tmin", C.c_double), ("tmax", C.c_double), ("emission_absorption", C.c_int32),
                ("stokes", C.c_int32), ("gamma", C.c_int32), ("reserved", C.c_int32)]


class Spectra(C.Structure):
    _fields_ = [("struct_size", C.c_int64)] + [(k, _F64P) for k in SPEC_OUTPUTS] + \
               [(k, _F32P) for k in ("lower_freq", "delta_freq", "gamma_lower_freq", "gamma_delta_freq")] + \
               [("nescaped_rpkt", C.c_int64), ("nescaped_gamma", C.c_int64)] + \
               [(k, C.c_int32) for k in ("ntimesteps", "ndirslots", "nelements", "max_nions", "proccount", "reserved")]


# engine configuration and layout plan (include/artis_amd.h artis_amd_config / artis_amd_plan)
class Config(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("cache_budget_bytes", C.c_int64), ("cache_headroom_bytes", C.c_int64),
                ("pop_scratch_bytes", C.c_int64), ("ma_hot_fraction", C.c_double), ("ma_pool_fraction", C.c_double),
                ("tail_threshold", C.c_int64), ("tile_park_at", C.c_int64), ("keep_line_dpop", C.c_int32), ("reserved", C.c_int32)]


# what artis_amd_config_default() writes: every field "automatic / default"
CONFIG_DEFAULTS = dict(cache_budget_bytes=0, cache_headroom_bytes=-1, pop_scratch_bytes=-1, ma_hot_fraction=-1.0, ma_pool_fraction=-1.0,
                       tail_threshold=-1, tile_park_at=-1, keep_line_dpop=-1, reserved=0)


def config(**fields) -> Config:
    """An artis_amd_config with the given fields set and every other one at "automatic / default"."""
    unknown = set(fields) - set(CONFIG_DEFAULTS)
    if unknown:
        raise TypeError(f"artis_amd_config has no field {sorted(unknown)}")
    return Config(struct_size=C.sizeof(Config), **{**CONFIG_DEFAULTS, **fields})


class Plan(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("bytes_per_cell", C.c_int64), ("cells_resident", C.c_int64), ("ntiles", C.c_int32),
                ("ncold_levels", C.c_int32), ("hot_fraction", C.c_double), ("pool_slots", C.c_int64), ("cache_bytes", C.c_int64),
                ("pool_bytes", C.c_int64), ("pop_scratch_bytes", C.c_int64), ("model_bytes", C.c_int64), ("free_bytes_assumed", C.c_int64),
                ("line_dpop_kept", C.c_int32), ("reserved", C.c_int32)]


def struct_dict(s: C.Structure) -> dict:
    return {k: getattr(s, k) for k, _ in s._fields_}


# radiation-field fit (include/artis_amd.h artis_amd_radfield_*)
RADFIELD_FITTED, RADFIELD_NUBAR_KEPT, RADFIELD_TJ_KEPT = 1, 2, 4
RADFIELD_TJ_LOW, RADFIELD_TJ_HIGH, RADFIELD_TR_LOW, RADFIELD_TR_HIGH = 8, 16, 32, 64
RADFIELD_COUNTS = ["trmin", "trmax", "retried", "zeroed", "notconverged"]  # ARTIS_RADFIELD_COUNT_* in index order


class RadfieldConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("prev_mid", C.c_double), ("deltat", C.c_double), ("nprocs", C.c_int32),
                ("lte_iteration", C.c_int32), ("assocvolume_tmin", _F64P), ("bfrate_normed_seed", _F32P)]


class Radfield(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("J", _F64P), ("nuJ", _F64P), ("J_normfactor", _F64P), ("TJ", _F32P), ("TR", _F32P),
                ("Te", _F32P), ("W", _F32P), ("flags", _I32P), ("cell_counts", _I32P), ("radfieldbin_T_R", _F32P),
                ("radfieldbin_W", _F32P), ("bfrate_normed", _F32P), ("Jb_lu_normed", _F64P), ("Jb_lu_contribcount", _I64P),
                ("totals", C.c_int64 * 5), ("npts_nonempty", C.c_int32), ("nbins", C.c_int32), ("nbfestim", C.c_int32),
                ("detailed_linecount", C.c_int32), ("kernel_ms", C.c_double * 2)]


def radfield_arrays(ncell: int, nbins: int, nbfestim: int, nlines: int) -> dict:
    """zeroed host arrays for every output of artis_radfield (the keys are its field names)"""
    out = dict(J=np.zeros(ncell), nuJ=np.zeros(ncell), J_normfactor=np.zeros(ncell), TJ=np.zeros(ncell, np.float32),
               TR=np.zeros(ncell, np.float32), Te=np.zeros(ncell, np.float32), W=np.zeros(ncell, np.float32),
               flags=np.zeros(ncell, np.int32), cell_counts=np.zeros((ncell, len(RADFIELD_COUNTS)), np.int32))
    if nbins:
        out.update(radfieldbin_T_R=np.zeros(ncell * nbins, np.float32), radfieldbin_W=np.zeros(ncell * nbins, np.float32))
    if nbfestim:
        out["bfrate_normed"] = np.zeros(ncell * nbfestim, np.float32)
    if nlines:
        out.update(Jb_lu_normed=np.zeros(ncell * nlines), Jb_lu_contribcount=np.zeros(ncell * nlines, np.int64))
    return out


def radfield_point(rf: Radfield, arrays: dict):
    """point the fields of rf at the arrays of radfield_arrays()"""
    types = dict(Radfield._fields_)
    for k, v in arrays.items():
        setattr(rf, k, v.ctypes.data_as(types[k]))


def radfield_config(prev_mid: float, deltat: float, nprocs: int, assocvolume_tmin: np.ndarray, lte_iteration: bool = False,
                    bfrate_normed_seed=None):
    """(RadfieldConfig, the arrays it points into: keep them alive while it is used)"""
    vol = np.ascontiguousarray(assocvolume_tmin, dtype=np.float64)
    seed = None if bfrate_normed_seed is None else np.ascontiguousarray(bfrate_normed_seed, dtype=np.float32)
    cfg = RadfieldConfig(struct_size=C.sizeof(RadfieldConfig), prev_mid=prev_mid, deltat=deltat, nprocs=nprocs,
                         lte_iteration=int(bool(lte_iteration)), assocvolume_tmin=vol.ctypes.data_as(_F64P),
                         bfrate_normed_seed=seed.ctypes.data_as(_F32P) if seed is not None else None)
    return cfg, (vol, seed)


# ionisation balance and hand-over of the grid update (include/artis_amd.h artis_amd_grid_update*)
IONBAL_NEUTRAL, IONBAL_MAXIT, IONBAL_PHI_OVERFLOW, IONBAL_FRAC_ZEROED = 1, 2, 4, 8
IONBAL_NOT_BRACKETED, IONBAL_INVALID_U, IONBAL_NONFINITE, IONBAL_FORCED_SAHA = 16, 32, 64, 128
IONBAL_FLAGS = ["neutral", "maxit", "phi_overflow", "frac_zeroed", "not_bracketed", "invalid_u", "nonfinite", "forced_saha"]
IONBAL_NTIMES = 4


class GridUpdate(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("use_fit", C.c_int32), ("TJ", _F32P), ("TR", _F32P), ("W", _F32P), ("Te", _F32P),
                ("rho", _F32P), ("elem_massfracs", _F32P), ("elem_meanweight", _F32P), ("thick", _I32P), ("kappagrey", _F32P),
                ("clumpfactor", _F32P), ("ffegrp", _F32P)]


class GridUpdateResult(C.Structure):
    _fields_ = [("struct_size", C.c_int64)] + [(k, _F32P) for k in ("Te", "TJ", "TR", "W", "nne", "nnetot", "rho", "ion_partfuncts",
                                                                      "ion_groundlevelpops")] + \
               [("uppermost_ion", _I32P), ("gamma_normed", _F64P), ("phi", _F64P), ("nne_root", _F32P), ("flags", _I32P), ("evals", _I32P),
                ("ncells_flagged", C.c_int64 * 8), ("total_evals", C.c_int64), ("npts_nonempty", C.c_int32), ("nions", C.c_int32),
                ("nelements", C.c_int32), ("nbfcontinua_ground", C.c_int32), ("kernel_ms", C.c_double * IONBAL_NTIMES)]


def grid_update_arrays(ncell: int, nions: int, nelements: int, nbfg: int) -> dict:
    """zeroed host arrays for every output of artis_grid_update_result (the keys are its field names)"""
    out = {k: np.zeros(ncell, np.float32) for k in ("Te", "TJ", "TR", "W", "nne", "nnetot", "rho", "nne_root")}
    out.update(ion_partfuncts=np.zeros(ncell * nions, np.float32), ion_groundlevelpops=np.zeros(ncell * nions, np.float32),
               uppermost_ion=np.zeros(ncell * nelements, np.int32), gamma_normed=np.zeros(max(ncell * nbfg, 1)), phi=np.zeros(ncell * nions),
               flags=np.zeros(ncell, np.int32), evals=np.zeros(ncell, np.int32))
    return out


def grid_update_config(use_fit: bool, rho, elem_massfracs, thick, elem_meanweight=None, TJ=None, TR=None, W=None, Te=None,
                       kappagrey=None, clumpfactor=None, ffegrp=None):
    """(GridUpdate, the arrays it points into: keep them alive while it is used); None: a NULL pointer"""
    keep = {}
    u = GridUpdate(struct_size=C.sizeof(GridUpdate), use_fit=int(bool(use_fit)))
    for k, v, dt, pt in (("TJ", TJ, np.float32, _F32P), ("TR", TR, np.float32, _F32P), ("W", W, np.float32, _F32P),
                         ("Te", Te, np.float32, _F32P), ("rho", rho, np.float32, _F32P), ("elem_massfracs", elem_massfracs, np.float32, _F32P),
                         ("elem_meanweight", elem_meanweight, np.float32, _F32P), ("thick", thick, np.int32, _I32P),
                         ("kappagrey", kappagrey, np.float32, _F32P), ("clumpfactor", clumpfactor, np.float32, _F32P),
                         ("ffegrp", ffegrp, np.float32, _F32P)):
        if v is None:
            continue
        keep[k] = np.ascontiguousarray(v, dtype=dt)
        setattr(u, k, keep[k].ctypes.data_as(pt))
    return u, keep


# decay and abundance update (include/artis_amd.h artis_amd_decay_*)
DECAYTYPE_ALPHA, DECAYTYPE_ELECTRONCAPTURE, DECAYTYPE_BETAPLUS, DECAYTYPE_BETAMINUS, DECAYTYPE_NONE, DECAYTYPE_SPONTFISSION = range(6)


class DecayModel(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("nnuclides", C.c_int32), ("npaths", C.c_int32), ("nuc_z", _I32P), ("nuc_a", _I32P),
                ("nuc_meanlife", _F64P), ("path_start", _I32P), ("path_nucindex", _I32P), ("path_branchproduct", _F64P),
                ("path_last_decaytype", _I32P), ("t_model", C.c_double), ("initnucmassfrac", _F32P),
                ("elem_untrackedstable_initmassfrac", _F32P), ("elem_initstablemeannucmass", _F32P), ("rho_tmin", _F32P)]


class DecayCoeffs(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("endnuc_coeff", _F64P), ("he4_coeff", _F64P), ("survivingfrac", _F64P)]


class DecayResult(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("rho", _F32P), ("elem_massfracs", _F32P), ("elem_meanweight", _F32P), ("endnuc_coeff", _F64P),
                ("he4_coeff", _F64P), ("survivingfrac", _F64P), ("path_scale", _F64P), ("path_x_dom", _F64P), ("nuc_massfracs", _F64P),
                ("npts_nonempty", C.c_int32), ("nelements", C.c_int32), ("nnuclides", C.c_int32), ("npaths", C.c_int32),
                ("he4_nucindex", C.c_int32), ("have_nuclides", C.c_int32), ("kernel_ms", C.c_double * 3), ("t_mid", C.c_double)]


_DECAY_MODEL_ARRAYS = (("nuc_z", np.int32), ("nuc_a", np.int32), ("nuc_meanlife", np.float64), ("path_start", np.int32),
                       ("path_nucindex", np.int32), ("path_branchproduct", np.float64), ("path_last_decaytype", np.int32),
                       ("initnucmassfrac", np.float32), ("elem_untrackedstable_initmassfrac", np.float32),
                       ("elem_initstablemeannucmass", np.float32), ("rho_tmin", np.float32))


def decay_model(d: dict):
    """(DecayModel, the arrays it points into: keep them alive while it is used) from a dict over artis_decay_model's fields
    (synth.decay_model); an array that is None or missing stays a NULL pointer"""
    types = dict(DecayModel._fields_)
    keep = {}
    m = DecayModel(struct_size=C.sizeof(DecayModel), nnuclides=len(d["nuc_z"]), npaths=len(d["path_start"]) - 1, t_model=float(d["t_model"]))
    for k, dt in _DECAY_MODEL_ARRAYS:
        if d.get(k) is None:
            continue
        a = np.ascontiguousarray(d[k], dtype=dt).reshape(-1)
        keep[k] = a if a.size else np.zeros(1, dt)
        setattr(m, k, keep[k].ctypes.data_as(types[k]))
    return m, keep


def decay_coeffs(endnuc_coeff, he4_coeff, survivingfrac):
    """(DecayCoeffs, the arrays it points into)"""
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (endnuc_coeff, he4_coeff, survivingfrac)]
    c = DecayCoeffs(struct_size=C.sizeof(DecayCoeffs), endnuc_coeff=keep[0].ctypes.data_as(_F64P), he4_coeff=keep[1].ctypes.data_as(_F64P),
                    survivingfrac=keep[2].ctypes.data_as(_F64P))
    return c, keep


def decay_arrays(ncell: int, nelements: int, nnuclides: int, npaths: int, nuclides: bool) -> dict:
    """zeroed host arrays for the outputs of artis_decay_result (the keys are its field names)"""
    out = dict(rho=np.zeros(ncell, np.float32), elem_massfracs=np.zeros(ncell * nelements, np.float32),
               elem_meanweight=np.zeros(ncell * nelements, np.float32), endnuc_coeff=np.zeros(npaths), he4_coeff=np.zeros(npaths),
               survivingfrac=np.zeros(nnuclides), path_scale=np.zeros(npaths), path_x_dom=np.zeros(npaths))
    if nuclides:
        out["nuc_massfracs"] = np.zeros(ncell * nnuclides)
    return out


# deposition rates and thickness (include/artis_amd.h artis_amd_deposition_*)
DEP_NCHANNELS, DEP_NVECTORS, DEP_NTOTALS = 5, 11, 15
CELL_THIN, CELL_THICK, CELL_THICK_VPKT_ONLY = 0, 1, 2  # ARTIS_CELL_*
DEP_CHANNELS = ("gamma", "positron", "electron", "alpha", "spfission")
DEP_VECTORS = DEP_CHANNELS + tuple(f"qdot_{k}" for k in ("alpha", "electroncapture", "betaplus", "betaminus", "none", "spfission"))
DEP_TOTALS = ("gamma_dep", "positron_dep", "electron_dep", "alpha_dep") + tuple(f"eps_{k}_ana_power" for k in DEP_CHANNELS) + DEP_VECTORS[5:]


class DepositionModel(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("nnuclides", C.c_int32), ("npts_nonempty", C.c_int32), ("nuc_endecay_gamma", _F64P),
                ("nuc_endecay_particle", _F64P), ("nuc_endecay_q", _F64P), ("nuc_branchprob", _F64P), ("assocvolume_tmin", _F64P),
                ("radial_pos_tmin", _F64P)]


class DepositionParams(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("mid", C.c_double), ("width", C.c_double), ("nts", C.c_int32), ("nprocs", C.c_int32),
                ("nts_next", C.c_int32), ("num_grey_timesteps", C.c_int32), ("optical_depth_is_thick", C.c_double),
                ("optical_depth_is_thick_vpkt", C.c_double), ("power_vectors", _F64P)]


class DepositionResult(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("eps_ana", _F64P), ("dep", _F64P), ("ntlepton_deposition_rate_density", _F64P),
                ("grey_depth", _F32P), ("thick", _I32P), ("power_vectors", _F64P), ("totmassnuclide", _F64P),
                ("totals", C.c_double * DEP_NTOTALS), ("mtot", C.c_double), ("npts_nonempty", C.c_int32), ("nnuclides", C.c_int32),
                ("nradioactive", C.c_int32), ("nts_next", C.c_int32), ("t_mid", C.c_double), ("kernel_ms", C.c_double * 3)]


_DEP_MODEL_ARRAYS = ("nuc_endecay_gamma", "nuc_endecay_particle", "nuc_endecay_q", "nuc_branchprob", "assocvolume_tmin", "radial_pos_tmin")


def deposition_model(d: dict):
    """(DepositionModel, the arrays it points into: keep them alive while it is used) from a dict over artis_deposition_model's array
    fields (synth.decay_energies, synth.assocvolume_tmin, synth.radial_pos_tmin); an array that is None or missing stays a NULL
    pointer; the counts are the arrays' unless the dict names them"""
    keep = {}
    m = DepositionModel(struct_size=C.sizeof(DepositionModel), nnuclides=int(d.get("nnuclides", len(d["nuc_endecay_gamma"]))),
                        npts_nonempty=int(d.get("npts_nonempty", len(d["assocvolume_tmin"]))))
    for k in _DEP_MODEL_ARRAYS:
        if d.get(k) is None:
            continue
        a = np.ascontiguousarray(d[k], dtype=np.float64).reshape(-1)
        keep[k] = a if a.size else np.zeros(1)
        setattr(m, k, keep[k].ctypes.data_as(_F64P))
    return m, keep


def deposition_params(mid: float, width: float, nts: int, nts_next: int, num_grey_timesteps: int, optical_depth_is_thick: float,
                      optical_depth_is_thick_vpkt: float = 0.0, nprocs: int = 1, power_vectors=None):
    """(DepositionParams, the array it points into)"""
    keep = None if power_vectors is None else np.ascontiguousarray(power_vectors, dtype=np.float64).reshape(-1)
    p = DepositionParams(struct_size=C.sizeof(DepositionParams), mid=mid, width=width, nts=nts, nprocs=nprocs, nts_next=nts_next,
                         num_grey_timesteps=num_grey_timesteps, optical_depth_is_thick=optical_depth_is_thick,
                         optical_depth_is_thick_vpkt=optical_depth_is_thick_vpkt,
                         power_vectors=keep.ctypes.data_as(_F64P) if keep is not None else None)
    return p, keep


def deposition_arrays(ncell: int, nnuclides: int) -> dict:
    """zeroed host arrays for the outputs of artis_deposition_result (the keys are its field names)"""
    return dict(eps_ana=np.zeros(DEP_NCHANNELS * ncell), dep=np.zeros(DEP_NCHANNELS * ncell), ntlepton_deposition_rate_density=np.zeros(ncell),
                grey_depth=np.zeros(ncell, np.float32), thick=np.zeros(ncell, np.int32), power_vectors=np.zeros(DEP_NVECTORS * nnuclides),
                totmassnuclide=np.zeros(nnuclides))


# pellet initialisation (include/artis_amd.h artis_amd_packet_init*)
PINIT_NKERNELS = 7
PINIT_KERNELS = ("energy", "checkpoints", "cumulative", "place", "decay", "normalise", "install")
PINIT_CHANNEL_UNSET = -2


class PacketInitModel(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("nuc_decay_daughters_probsum", _F64P), ("gamma_start", _I32P), ("gamma_energy", _F64P),
                ("gamma_probability", _F64P), ("initenergyq", _F64P), ("tmax", C.c_double), ("initial_packets_on", C.c_int32),
                ("use_model_initial_energy", C.c_int32), ("uniform_pellet_energies", C.c_int32), ("max_trials_per_launch", C.c_int32)]


class PacketInitResult(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("en_cumulative", _F64P), ("energy_vector", _F64P), ("endecay_per_mass", _F64P), ("channel", _I32P),
                ("trials", _I32P), ("npackets", C.c_int64), ("ngrid", C.c_int32), ("npts_nonempty", C.c_int32), ("npaths", C.c_int32),
                ("ncheckpoints", C.c_int32), ("etot_simtime", C.c_double), ("e_cmf_per_packet", C.c_double), ("e_cmf_total", C.c_double),
                ("e_ratio", C.c_double), ("continuation_launches", C.c_int32), ("max_trials", C.c_int32), ("kernel_ms", C.c_double * PINIT_NKERNELS)]


_PINIT_MODEL_ARRAYS = (("nuc_decay_daughters_probsum", np.float64), ("gamma_start", np.int32), ("gamma_energy", np.float64),
                       ("gamma_probability", np.float64), ("initenergyq", np.float64))


def packet_init_model(d: dict):
    """(PacketInitModel, the arrays it points into: keep them alive while it is used) from a dict over artis_packet_init_model's fields
    (synth.packet_init_model); an array that is None or missing stays a NULL pointer, a switch that is missing takes the value most
    option sets have (initial packets off, uniform pellet energies on, the default trial budget)"""
    types = dict(PacketInitModel._fields_)
    keep = {}
    m = PacketInitModel(struct_size=C.sizeof(PacketInitModel), tmax=float(d["tmax"]), initial_packets_on=int(d.get("initial_packets_on", 0)),
                        use_model_initial_energy=int(d.get("use_model_initial_energy", 0)), uniform_pellet_energies=int(d.get("uniform_pellet_energies", 1)),
                        max_trials_per_launch=int(d.get("max_trials_per_launch", 0)))
    for k, dt in _PINIT_MODEL_ARRAYS:
        if d.get(k) is None:
            continue
        a = np.ascontiguousarray(d[k], dtype=dt).reshape(-1)
        keep[k] = a if a.size else np.zeros(1, dt)
        setattr(m, k, keep[k].ctypes.data_as(types[k]))
    return m, keep


def packet_init_arrays(ngrid: int, ncell: int, npaths: int, npackets: int) -> dict:
    """zeroed host arrays for the outputs of artis_packet_init_result (the keys are its field names)"""
    return dict(en_cumulative=np.zeros(ngrid), energy_vector=np.zeros(npaths), endecay_per_mass=np.zeros(ncell), channel=np.zeros(npackets, np.int32),
                trials=np.zeros(npackets, np.int32))


# initial temperatures and the first cell state (include/artis_amd.h artis_amd_initial_state*)
GREY_FEGROUP_APPROX, GREY_TANAKA2020, GREY_JUST2022 = 0, 1, 2
INITIAL_INSIDE, INITIAL_BELOW_MINTEMP, INITIAL_ABOVE_MAXTEMP, INITIAL_NONFINITE = 0, 1, 2, 3
INITIAL_BRANCH_MASK, INITIAL_KAPPA_INVALID = 3, 4
INITIAL_BRANCHES = ("inside", "below_mintemp", "above_maxtemp", "nonfinite")
INITIAL_KERNELS = ("energy", "cells")


class InitialParams(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("tstart", C.c_double), ("nts_first", C.c_int32), ("num_grey_timesteps", C.c_int32),
                ("optical_depth_is_thick", C.c_double), ("optical_depth_is_thick_vpkt", C.c_double), ("rpkt_grey_type", C.c_int32),
                ("mfegroup", C.c_double), ("mtot_input", C.c_double), ("ffegrp", _F32P), ("initelectronfrac", _F32P), ("energy_vector", _F64P)]


class InitialResult(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("T_initial", _F32P), ("endecay_per_mass", _F64P), ("kappagrey", _F32P), ("grey_depth", _F32P),
                ("thick", _I32P), ("flags", _I32P), ("energy_vector", _F64P), ("path_scale", _F64P), ("path_x_dom", _F64P),
                ("ncells_branch", C.c_int64 * 4), ("ncells_kappa_invalid", C.c_int64), ("first_nonfinite_cell", C.c_int32),
                ("npts_nonempty", C.c_int32), ("npaths", C.c_int32), ("rpkt_grey_type", C.c_int32), ("nts_first", C.c_int32),
                ("reserved", C.c_int32), ("first_nonfinite_rho_tmin", C.c_double), ("first_nonfinite_endecay", C.c_double),
                ("tstart", C.c_double), ("kernel_ms", C.c_double * 2)]


def initial_params(d: dict):
    """(InitialParams, the arrays it points into: keep them alive while it is used) from a dict over artis_initial_params's fields
    (synth.initial_model plus tstart and the step's numbers); an array that is None or missing stays a NULL pointer"""
    keep = {}
    p = InitialParams(struct_size=C.sizeof(InitialParams), tstart=float(d["tstart"]), nts_first=int(d.get("nts_first", 0)),
                      num_grey_timesteps=int(d.get("num_grey_timesteps", 0)), optical_depth_is_thick=float(d.get("optical_depth_is_thick", 0.0)),
                      optical_depth_is_thick_vpkt=float(d.get("optical_depth_is_thick_vpkt", 0.0)), rpkt_grey_type=int(d.get("rpkt_grey_type", 0)),
                      mfegroup=float(d.get("mfegroup", 0.0)), mtot_input=float(d.get("mtot_input", 0.0)))
    for k, dt, pt in (("ffegrp", np.float32, _F32P), ("initelectronfrac", np.float32, _F32P), ("energy_vector", np.float64, _F64P)):
        if d.get(k) is None:
            continue
        a = np.ascontiguousarray(d[k], dtype=dt).reshape(-1)
        keep[k] = a if a.size else np.zeros(1, dt)
        setattr(p, k, keep[k].ctypes.data_as(pt))
    return p, keep


def initial_arrays(ncell: int, npaths: int) -> dict:
    """zeroed host arrays for the outputs of artis_initial_result (the keys are its field names)"""
    return dict(T_initial=np.zeros(ncell, np.float32), endecay_per_mass=np.zeros(ncell), kappagrey=np.zeros(ncell, np.float32),
                grey_depth=np.zeros(ncell, np.float32), thick=np.zeros(ncell, np.int32), flags=np.zeros(ncell, np.int32),
                energy_vector=np.zeros(npaths), path_scale=np.zeros(npaths), path_x_dom=np.zeros(npaths))


# thermal balance of the thin cells (include/artis_amd.h artis_amd_thermal_*)
THERMAL_BRACKETED, THERMAL_PINNED_LOW, THERMAL_PINNED_HIGH, THERMAL_NONFINITE = 256, 512, 1024, 2048
THERMAL_DAMPED_UP, THERMAL_DAMPED_DOWN, THERMAL_MAXIT, THERMAL_RENORM_ONE = 4096, 8192, 16384, 32768
THERMAL_FLAGS = IONBAL_FLAGS + ["bracketed", "pinned_low", "pinned_high", "nonfinite_ends", "damped_up", "damped_down", "maxit", "renorm_one"]
THERMAL_NRATES = 10
THERMAL_NTIMES = 4
THERMAL_RATES = ("cooling_ff", "cooling_collisional", "cooling_fb", "cooling_adiabatic", "heating_ff", "heating_bf", "heating_collisional",
                 "heating_dep", "residual", "dep_frac_heating")
THERMAL_KERNELS = ("renorm", "gamma_partfunct", "solve", "rates")


class ThermalParams(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("rho", _F32P), ("elem_massfracs", _F32P), ("elem_meanweight", _F32P), ("bfheatingcoeffs", _F64P),
                ("ntlepton_dep", _F64P), ("dep_alpha", _F64P), ("dep_spfission", _F64P), ("clumpfactor", _F32P)]


class ThermalResult(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("Te", _F32P), ("Te_solved", _F64P), ("bracket", _F64P), ("evals", _I32P), ("flags", _I32P),
                ("nne", _F32P), ("rates", _F64P), ("ion_groundlevelpops", _F32P), ("ion_partfuncts", _F32P), ("phi", _F64P), ("gamma", _F64P),
                ("corrphotoionrenorm", _F64P), ("ncells_flagged", C.c_int64 * len(THERMAL_FLAGS)), ("total_evals", C.c_int64),
                ("nfitted", C.c_int64), ("npts_nonempty", C.c_int32), ("nions", C.c_int32), ("nbfcontinua_ground", C.c_int32),
                ("nlevels", C.c_int32), ("kernel_ms", C.c_double * THERMAL_NTIMES)]


def thermal_params(bfheatingcoeffs, rho=None, elem_massfracs=None, elem_meanweight=None, ntlepton_dep=None, dep_alpha=None,
                   dep_spfission=None, clumpfactor=None):
    """(ThermalParams, the arrays it points into: keep them alive while it is used); None: a NULL pointer"""
    keep = {}
    p = ThermalParams(struct_size=C.sizeof(ThermalParams))
    for k, v, dt, pt in (("rho", rho, np.float32, _F32P), ("elem_massfracs", elem_massfracs, np.float32, _F32P),
                         ("elem_meanweight", elem_meanweight, np.float32, _F32P), ("bfheatingcoeffs", bfheatingcoeffs, np.float64, _F64P),
                         ("ntlepton_dep", ntlepton_dep, np.float64, _F64P), ("dep_alpha", dep_alpha, np.float64, _F64P),
                         ("dep_spfission", dep_spfission, np.float64, _F64P), ("clumpfactor", clumpfactor, np.float32, _F32P)):
        if v is None:
            continue
        keep[k] = np.ascontiguousarray(v, dtype=dt).reshape(-1)
        setattr(p, k, keep[k].ctypes.data_as(pt))
    return p, keep


def thermal_arrays(ncell: int, nions: int, nbfg: int) -> dict:
    """zeroed host arrays for every output of artis_thermal_result (the keys are its field names)"""
    return dict(Te=np.zeros(ncell, np.float32), Te_solved=np.zeros(ncell), bracket=np.zeros(2 * ncell), evals=np.zeros(ncell, np.int32),
                flags=np.zeros(ncell, np.int32), nne=np.zeros(ncell, np.float32), rates=np.zeros(ncell * THERMAL_NRATES),
                ion_groundlevelpops=np.zeros(ncell * nions, np.float32), ion_partfuncts=np.zeros(ncell * nions, np.float32),
                phi=np.zeros(ncell * nions), gamma=np.zeros(max(ncell * nbfg, 1)), corrphotoionrenorm=np.zeros(max(ncell * nbfg, 1)))


# bound-free heating coefficients of the thin cells (include/artis_amd.h artis_amd_bfheating_*)
BFHEAT_RENORM_ONE, BFHEAT_NONFINITE = 1, 2
BFHEAT_NTOTALS = 3
BFHEAT_NTIMES = 2
BFHEAT_TOTALS = ("nodes", "subdivided", "at_depth_cap")
BFHEAT_KERNELS = ("ground", "levels")


class BfheatingParams(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("TR", _F32P), ("W", _F32P)]


class BfheatingResult(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("coeffs", _F64P), ("renorm", _F64P), ("flags", _I32P), ("totals", C.c_int64 * BFHEAT_NTOTALS),
                ("nfitted", C.c_int64), ("nintegrals", C.c_int64), ("npts_nonempty", C.c_int32), ("nlevels", C.c_int32),
                ("nbfcontinua_ground", C.c_int32), ("nlevels_with_targets", C.c_int32), ("kernel_ms", C.c_double * BFHEAT_NTIMES)]


class Gk61Case(C.Structure):
    _fields_ = [("which", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double), ("a", C.c_double), ("b", C.c_double), ("tol", C.c_double)]


class Gk61Result(C.Structure):
    _fields_ = [("result", C.c_double), ("error", C.c_double), ("evals", C.c_int64), ("nodes", C.c_int32), ("maxdepth", C.c_int32)]


def bfheating_params(TR=None, W=None):
    """(BfheatingParams, the arrays it points into: keep them alive while it is used); None: a NULL pointer (the last fit's)"""
    keep = {}
    p = BfheatingParams(struct_size=C.sizeof(BfheatingParams))
    for k, v in (("TR", TR), ("W", W)):
        if v is None:
            continue
        keep[k] = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
        setattr(p, k, keep[k].ctypes.data_as(_F32P))
    return p, keep


# rate-coefficient tables (include/artis_amd.h artis_amd_ratecoeff_*)
RATECOEFF_BAD_ALPHA_SP, RATECOEFF_BAD_GAMMACORR, RATECOEFF_BAD_BFCOOLING, RATECOEFF_BAD_SAHAFACT = 1, 2, 4, 8


class RatecoeffRequest(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("install", C.c_int32), ("reserved", C.c_int32), ("items_per_launch", C.c_int64)]


class RatecoeffStats(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("integrals", C.c_int64), ("nodes", C.c_int64), ("at_depth_cap", C.c_int64), ("flagged", C.c_int64),
                ("first_flagged", C.c_int64), ("nbfcontinua", C.c_int64), ("ncovered", C.c_int64), ("tablesize", C.c_int32), ("ntables", C.c_int32),
                ("kernel_ms", C.c_double)]


# photoionisation coefficients of builds without USE_LUT_PHOTOION (include/artis_amd.h artis_amd_set_cellstate_photoion)
PHOTOION_NONFINITE = 1
PHOTOION_SRC_ESTIMATOR, PHOTOION_SRC_INTEGRAL = 1, 2
PHOTOION_NTOTALS = 5
PHOTOION_TOTALS = ("from_estimators", "integrals", "nodes", "at_depth_cap", "nonfinite")


class PhotoionParams(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("use_bf_estimators", C.c_int32), ("bfrate_normed", _F32P), ("cells_per_launch", C.c_int32)]


class PhotoionResult(C.Structure):
    _fields_ = [("struct_size", C.c_int64), ("coeff", _F64P), ("source", C.POINTER(C.c_uint8)), ("flags", _I32P),
                ("totals", C.c_int64 * PHOTOION_NTOTALS), ("npts_nonempty", C.c_int32), ("nphixstargets_total", C.c_int32),
                ("nbfcontinua", C.c_int32), ("nbfestim", C.c_int32), ("kernel_ms", C.c_double)]
