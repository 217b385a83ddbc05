"""The per-packet rules of the device spectra (artis_amd/csrc/spectra.h) compiled for x86 (tests/spectra_host) and summed in packet
order, against the numpy restatements of tools/exspec.py: bit for bit, on oracle-made populations and on hand-made edge packets."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
import exspec  # noqa: E402
import host_build  # noqa: E402
from artis_amd import abi, synth  # noqa: E402

_HOSTDIR = os.path.join(HERE, "spectra_host")
_LIB = []
NU_MIN, NU_MAX = 1e14, 5e15  # classic build (include/artis_options.h ARTIS_OPT_NU_MIN_R / _MAX_R)
WIDTH = 0.05


def _lib():
    if not _LIB:
        L = host_build.load(_HOSTDIR, lambda p: "libspectra_host.so", "classic")
        L.spec_host_emission_column.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.spec_host_compute.restype = C.c_int64
        L.spec_host_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(abi.SpectraConfig), C.c_double, C.c_double, C.c_int,
                                        C.POINTER(C.POINTER(C.c_double)), C.c_void_p]
        _LIB.append(L)
    return _LIB[0]


def host_spectra(model, pk, starts, widths, tmin, tmax, dirbin=-1, emission_absorption=False, stokes=False, gamma=False, nbf=-1):
    """the harness: the same outputs as Engine.spectra() (numpy shapes of artis_amd/engine.py)"""
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    widths = np.ascontiguousarray(widths, dtype=np.float64)
    T, B = len(starts), exspec.MNUBINS
    mx = exspec.max_nions(model)
    P, A = 2 * model["nelements"] * mx + 1, model["nelements"] * mx
    lead = (1 + exspec.MABINS,) if dirbin == abi.SPEC_ALL_DIRBINS else ()
    shapes = {"lum": (T,), "lumcmf": (T,), "flux": (B, T)}
    if stokes:
        shapes.update(flux_q=(B, T), flux_u=(B, T))
    if emission_absorption:
        shapes.update(emission=(B, T, P), trueemission=(B, T, P), absorption=(B, T, A))
        if stokes:
            shapes.update(emission_q=(B, T, P), emission_u=(B, T, P), absorption_q=(B, T, A), absorption_u=(B, T, A))
    out = {k: np.zeros(lead + v) for k, v in shapes.items()}
    if gamma:
        out.update(gamma_lum=np.zeros(T), gamma_lumcmf=np.zeros(T), gamma_flux=np.zeros((B, T)))
    ptrs = (C.POINTER(C.c_double) * len(abi.SPEC_OUTPUTS))()
    for i, k in enumerate(abi.SPEC_OUTPUTS):
        if k in out:
            ptrs[i] = out[k].ctypes.data_as(C.POINTER(C.c_double))
    grids = np.zeros(4 * B, dtype=np.float32)
    cfg = abi.SpectraConfig(struct_size=C.sizeof(abi.SpectraConfig), ntimesteps=T, dirbin=dirbin,
                            ts_start=starts.ctypes.data_as(C.POINTER(C.c_double)), ts_width=widths.ctypes.data_as(C.POINTER(C.c_double)),
                            tmin=tmin, tmax=tmax, emission_absorption=int(emission_absorption), stokes=int(stokes), gamma=int(gamma))
    pk = np.ascontiguousarray(pk)
    out["nescaped"] = int(_lib().spec_host_compute(C.cast(model.ref(), C.c_void_p), abi.packets_ptr(pk), len(pk), C.byref(cfg),
                                                    NU_MIN, NU_MAX, nbf, ptrs, grids.ctypes.data))
    out["lower_freq"], out["delta_freq"] = grids[:B], grids[B:2 * B]
    out["gamma_lower_freq"], out["gamma_delta_freq"] = grids[2 * B:3 * B], grids[3 * B:]
    return out


@pytest.fixture(scope="module")
def population(oracle):
    """~2e4 packets (r-, k-, gamma packets and pellets) through 4 consecutive timesteps of the oracle"""
    model, cs0, _, aux = synth.build("small", ncoord=8, nts=10)
    nsteps = 4
    pk = synth.make_packets(model, aux, 20000, kpkt_fraction=0.2, gamma_fraction=0.1, pellet_fraction=0.3,
                            ts_width_frac=(1.0 + WIDTH) ** nsteps - 1.0)
    n, g = model["npts_nonempty"], model["nbfcontinua_ground"]
    t, starts, widths = aux["t"], [], []
    for i in range(nsteps):
        ts = synth.make_timestep(t, width_frac=WIDTH, vmax=model["vmax"], nts=10 + i)
        oracle.update_packets(model, synth.evolve_cellstate(cs0, aux["t"], ts.c.mid), ts, pk, abi.Estimators(n, g))
        starts.append(ts.c.start)
        widths.append(ts.c.width)
        t = ts.c.start + ts.c.width
    starts, widths = np.array(starts), np.array(widths)
    # a wider time grid than the run: one timestep before it and one after, so that every rule of get_timestep is met
    starts = np.concatenate([[starts[0] * 0.9], starts, [t]])
    widths = np.concatenate([[starts[1] - starts[0]], widths, [0.1 * t]])
    return model, pk, starts, widths, starts[0], starts[-1] + widths[-1]


def _assert_same(a, b, keys, what):
    for k in keys:
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), (what, k, np.abs(a[k] - b[k]).max())


def _top_dirbins(pk):
    esc = (pk["type"] == abi.TYPE_ESCAPE) & (pk["escape_type"] == abi.TYPE_RPKT)
    counts = np.bincount(exspec.escapedirectionbin(pk["dir"][esc]), minlength=exspec.MABINS)
    return [int(b) for b in np.argsort(counts)[-3:]] + [0, 55]


def test_flux_and_lightcurves_match_exspec(population):
    model, pk, starts, widths, tmin, tmax = population
    for b in [-1] + _top_dirbins(pk):
        h = host_spectra(model, pk, starts, widths, tmin, tmax, dirbin=b)
        r = exspec.spectrum_and_lightcurve(pk, starts, widths, tmin, tmax, model["vmax"], NU_MIN, NU_MAX, dirbin=b)
        _assert_same(h, r, ("flux", "lum", "lumcmf", "lower_freq", "delta_freq"), f"dirbin {b}")
        if b == -1:
            assert h["nescaped"] == r["nescaped"] > 1000
            assert np.count_nonzero(h["flux"]) > 500


def test_emission_absorption_and_stokes_match_exspec(population):
    model, pk, starts, widths, tmin, tmax = population
    for b in (-1, _top_dirbins(pk)[-3]):
        h = host_spectra(model, pk, starts, widths, tmin, tmax, dirbin=b, emission_absorption=True, stokes=True)
        r = exspec.stokes_and_emission_absorption(pk, starts, widths, tmin, tmax, model, NU_MIN, NU_MAX, dirbin=b)
        keys = ("flux_q", "flux_u", "emission", "emission_q", "emission_u", "trueemission", "absorption", "absorption_q", "absorption_u")
        _assert_same(h, r, keys, f"dirbin {b}")
        if b == -1:
            assert np.count_nonzero(h["absorption"]) > 50 and np.count_nonzero(h["emission"]) > 500
            assert np.count_nonzero(h["flux_q"]) > 100  # the classic build is POL_ON: scatterings polarise


def test_gamma_outputs_match_exspec(population):
    model, pk, starts, widths, tmin, tmax = population
    h = host_spectra(model, pk, starts, widths, tmin, tmax, gamma=True)
    r = exspec.gamma_spectrum_and_lightcurve(pk, starts, widths, tmin, tmax, model["vmax"])
    _assert_same(h, r, ("gamma_lum", "gamma_lumcmf", "gamma_flux", "gamma_lower_freq", "gamma_delta_freq"), "gamma")
    assert r["nescaped_gamma"] > 50 and h["gamma_lum"].sum() > 0


def test_all_dirbins_is_the_stack_of_single_dirbins(population):
    model, pk, starts, widths, tmin, tmax = population
    h = host_spectra(model, pk, starts, widths, tmin, tmax, dirbin=abi.SPEC_ALL_DIRBINS)
    r = exspec.all_dirbins(exspec.spectrum_and_lightcurve, pk, starts, widths, tmin, tmax, model["vmax"], NU_MIN, NU_MAX)
    _assert_same(h, r, ("flux", "lum", "lumcmf"), "all dirbins")
    # the 100 direction bins average to the angle average (each counts MABINS-fold, :562)
    for k in ("flux", "lum", "lumcmf"):
        assert np.allclose(h[k][1:].mean(axis=0), h[k][0], rtol=1e-12, atol=1e-300), k


def test_sum_rules(population):
    model, pk, starts, widths, tmin, tmax = population
    h = host_spectra(model, pk, starts, widths, tmin, tmax, emission_absorption=True)
    # exspec.cc:110-128: the frequency-integrated flux of a timestep never exceeds its light curve
    lum_from_spec = (h["flux"] * h["delta_freq"][:, None].astype(np.float64)).sum(axis=0) * 4.e12 * np.pi * exspec.PARSEC**2
    assert np.all(lum_from_spec <= h["lum"] * 1.001)
    assert lum_from_spec.sum() > 0.5 * h["lum"].sum()
    # the emission columns add up to the flux of the packets with an emission type (EMTYPE_NOTSET packets are not in a column)
    esc = pk[(pk["type"] == abi.TYPE_ESCAPE) & (pk["escape_type"] == abi.TYPE_RPKT)]
    notset = esc[esc["emissiontype"] == abi.EMTYPE_NOTSET]
    f_notset = exspec.spectrum_and_lightcurve(notset, starts, widths, tmin, tmax, model["vmax"], NU_MIN, NU_MAX)["flux"]
    assert np.allclose(h["emission"].sum(axis=2) + f_notset, h["flux"], rtol=1e-12, atol=1e-300)
    # trueemission: every packet with a true emission type
    assert np.all(h["trueemission"].sum(axis=2) <= h["flux"] * (1 + 1e-12))


def test_emission_columns_against_the_levels():
    """columnindex_from_emissiontype (spectrum_lightcurve.cc:168-203) against a direct loop over the model's levels and lines"""
    model = synth.build("small", ncoord=8)[0]
    L = _lib()
    nel, mx = model["nelements"], exspec.max_nions(model)
    seen = np.zeros(model["nbfcontinua"], dtype=int)
    for ui in range(model["nions"]):
        el = int(model["ion_element"][ui])
        ion = ui - int(model["elem_uniqueionindexstart"][el])
        l0 = int(model["ion_uniquelevelindexstart"][ui])
        for lv in range(int(model["ion_nlevels_ionising"][ui])):
            for t in range(int(model["level_nphixstargets"][l0 + lv])):
                bf = int(model["level_bflist_start"][l0 + lv]) + t
                seen[bf] += 1
                et = -1 - bf  # get_emtype_continuum (atomic.h:508)
                assert L.spec_host_emission_column(C.cast(model.ref(), C.c_void_p), et, -1) == nel * mx + el * mx + ion
                assert L.spec_host_emission_column(C.cast(model.ref(), C.c_void_p), et, 0) == 2 * nel * mx  # no bf continua
    assert np.all(seen == 1)  # every bflist entry belongs to one (level, target)
    for line in range(0, model["nlines"], max(1, model["nlines"] // 200)):
        want = int(model["line_elementindex"][line]) * mx + int(model["line_ionindex"][line])
        assert L.spec_host_emission_column(C.cast(model.ref(), C.c_void_p), line, -1) == want
    assert L.spec_host_emission_column(C.cast(model.ref(), C.c_void_p), abi.EMTYPE_FREEFREE, -1) == 2 * nel * mx
    assert L.spec_host_emission_column(C.cast(model.ref(), C.c_void_p), abi.EMTYPE_NOTSET, -1) == -1
    ets = np.array([0, model["nlines"] - 1, abi.EMTYPE_FREEFREE, abi.EMTYPE_NOTSET, -1, -model["nbfcontinua"]])
    want = [L.spec_host_emission_column(C.cast(model.ref(), C.c_void_p), int(e), -1) for e in ets]
    assert list(exspec.emission_columns(ets, model)) == want


def _edge_packets(model, starts, widths, tmin, tmax):
    """hand-made escaped packets on the edges of every rule"""
    dlognu, lower, delta = exspec._grid(NU_MIN, NU_MAX)
    t0 = starts[2]
    rows = []

    def add(**kw):
        p = dict(type=abi.TYPE_ESCAPE, escape_type=abi.TYPE_RPKT, escape_time=np.float32(t0 * 1.01), pos=(0., 0., 0.),
                 dir=(0.6, 0.0, 0.8), nu_rf=3e14, e_rf=1e40, e_cmf=0.9e40, emissiontype=0, trueemissiontype=1,
                 absorptiontype=2, absorptionfreq=4e14, stokes_q=0.3, stokes_u=-0.2)
        p.update(kw)
        rows.append(p)

    for nu in (NU_MIN, np.nextafter(NU_MIN, 1e30), np.nextafter(NU_MIN, 0), NU_MAX, np.nextafter(NU_MAX, 0), np.nextafter(NU_MAX, 1e30),
               float(lower[500]), float(lower[999])):
        add(nu_rf=nu)
    for t in (starts[1], starts[3], tmin, tmax, np.nextafter(tmin, 1e30)):  # t_arrive on an edge (escape_time is float32: via pos)
        et = np.float32(t * 1.001)
        add(escape_time=et, pos=(0., 0., (float(et) - t) * exspec.CLIGHT), dir=(0., 0., 1.))
    for d in ((0., 0., 1.), (0., 0., -1.), (0., 1e-14, 1.), (-1., 0., 0.), (0., -1., 0.), (0.3, -0.4, 0.5)):
        add(dir=d)
    nbf = model["nbfcontinua"]
    for et in (abi.EMTYPE_NOTSET, abi.EMTYPE_FREEFREE, -1, -nbf, -1 - nbf // 2):
        add(emissiontype=et, trueemissiontype=et)
    for at, af in ((-1, 4e14), (-2, 4e14), (5, NU_MAX * 2), (5, NU_MIN), (5, np.nextafter(NU_MIN, 1e30)), (model["nlines"] - 1, 1e15)):
        add(absorptiontype=at, absorptionfreq=af)
    add(escape_type=abi.TYPE_GAMMA, nu_rf=1e20)
    add(escape_type=abi.TYPE_GAMMA, nu_rf=exspec.NU_MIN_GAMMA)
    add(type=abi.TYPE_RPKT)       # not escaped
    add(type=abi.TYPE_KPKT)
    add(escape_type=abi.TYPE_KPKT)  # escaped, but neither an r-packet nor a gamma packet
    pk = np.zeros(len(rows), dtype=abi.PACKET_DTYPE)
    for i, r in enumerate(rows):
        for k, v in r.items():
            pk[k][i] = v
    return pk


@pytest.mark.parametrize("nbf", [-1, 0])
def test_edge_packets(population, nbf):
    model, pk_pop, starts, widths, tmin, tmax = population
    pk = _edge_packets(model, starts, widths, tmin, tmax)
    nbfc = None if nbf < 0 else 0
    for b in (-1, 0, 9, 90, 99, abi.SPEC_ALL_DIRBINS):
        h = host_spectra(model, pk, starts, widths, tmin, tmax, dirbin=b, emission_absorption=True, stokes=True, gamma=True, nbf=nbf)
        if b == abi.SPEC_ALL_DIRBINS:
            r = exspec.all_dirbins(exspec.spectrum_and_lightcurve, pk, starts, widths, tmin, tmax, model["vmax"], NU_MIN, NU_MAX)
            r.update(exspec.all_dirbins(exspec.stokes_and_emission_absorption, pk, starts, widths, tmin, tmax, model, NU_MIN, NU_MAX,
                                        nbfcontinua=nbfc))
        else:
            r = exspec.spectrum_and_lightcurve(pk, starts, widths, tmin, tmax, model["vmax"], NU_MIN, NU_MAX, dirbin=b)
            r.update(exspec.stokes_and_emission_absorption(pk, starts, widths, tmin, tmax, model, NU_MIN, NU_MAX, dirbin=b,
                                                           nbfcontinua=nbfc))
        r.update(exspec.gamma_spectrum_and_lightcurve(pk, starts, widths, tmin, tmax, model["vmax"]))
        keys = [k for k in abi.SPEC_OUTPUTS if k in h]
        _assert_same(h, r, keys, f"edge packets dirbin {b} nbf {nbf}")
    assert h["nescaped"] == int(np.count_nonzero((pk["type"] == abi.TYPE_ESCAPE) & (pk["escape_type"] == abi.TYPE_RPKT)))
    # the packets on the two ends of the frequency range, the three outside it and the not-escaped ones do not count
    assert np.count_nonzero(h["flux"][0]) > 0 and h["gamma_lum"].sum() > 0


def test_unfilled_bflist_entry_is_not_counted():
    """a bound-free emission type whose bflist entry no (level, target) fills counts in no column, on both sides"""
    model = synth.build("small", ncoord=8)[0]
    L = _lib()
    ls = np.nonzero(model["level_nphixstargets"] > 0)[0]
    lv = int(ls[len(ls) // 2])
    bf = int(model["level_bflist_start"][lv])
    et = -1 - bf
    assert L.spec_host_emission_column(C.cast(model.ref(), C.c_void_p), et, -1) >= 0
    model["level_nphixstargets"][lv] = 0  # (the struct points at this array)
    assert L.spec_host_emission_column(C.cast(model.ref(), C.c_void_p), et, -1) == -1
    assert exspec.emission_columns(np.array([et]), model)[0] == -1
