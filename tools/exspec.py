#!/usr/bin/env python3
"""Emergent spectrum and light curve of a packet array, binned by the reference's rules.

Host-side post-processing (the reference's exspec / write_partial_lightcurve_spectra, spectrum_lightcurve.cc), NOT part
of the packet path and not used by the engine: it turns the engine's (or the oracle's) escaped packets into the
artefact the reference compares runs by -- spec.out / light_curve.out -- so that a reference run of the same model can
be laid next to an engine run as soon as one exists. Angle-averaged (dirbin = -1) or one of the MABINS = 100 equal-solid-angle
direction bins of the reference (dirbin >= 0), one rank (nprocs_exspec = 1).

Rules restated (file:line of the reference):
  * a packet counts if type == TYPE_ESCAPE and escape_type == TYPE_RPKT              spectrum_lightcurve.cc:254-257
  * arrival time  t_arrive = escape_time - dot(pos, dir) / c                          :555 / :695
  * time bin = the timestep [start, next start) containing t_arrive                   :209 get_timestep
  * MNUBINS = 1000 log-spaced frequency bins over (nu_min, nu_max); index
    clamp(floor((ln nu - ln nu_min) / dlognu), 0, MNUBINS-1); edges stored as float32 exspec.h:8, sn3d.h:134-144, :487-504
  * flux += e_rf / width[nts] / delta_freq[nnu] / 4e12 / pi / PARSEC^2                :563  [erg/s/cm^2/Hz at 1 Mpc]
  * luminosity light curve  L[nts] += e_rf / width[nts]                               :698
  * comoving light curve  t_cmf = escape_time * sqrt(1 - vmax^2/c^2):
    Lcmf[nts] += e_cmf / width[nts] / sqrt(1 - vmax^2/c^2)                            :702-711
  * direction-resolved (dirbin >= 0): only packets with get_escapedirectionbin(dir) == dirbin, every contribution times
    MABINS (a bin sees 1/MABINS of the sphere)                                        :545, :562, :689-691; vectors.h:147
"""
from __future__ import annotations

import numpy as np

CLIGHT = 2.99792458e10
PARSEC = 3.0857e18  # constants.h
MNUBINS = 1000
TYPE_ESCAPE, TYPE_RPKT = 32, 11
NPHIBINS, NCOSTHETABINS = 10, 10  # exspec.h:10-11
MABINS = NPHIBINS * NCOSTHETABINS  # exspec.h:12


def escapedirectionbin(dirs: np.ndarray) -> np.ndarray:
    """get_escapedirectionbin (vectors.h:147) for an [n, 3] array of directions: costheta bin (about syn_dir = z, constants.h:94) *
    NPHIBINS + phi bin, the phi bins in decreasing phi order."""
    d = np.asarray(dirs, dtype=np.float64)
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    syn = np.array([0., 0., 1.])
    xhat = np.array([1., 0., 0.])
    costheta = d @ syn
    costhetabin = np.clip(((costheta + 1.0) * NCOSTHETABINS / 2.0).astype(np.int64), 0, NCOSTHETABINS - 1)
    vec1 = np.cross(d, syn)
    vec2 = np.cross(xhat, syn)
    vec1_len = np.sqrt((vec1 * vec1).sum(axis=1))
    safe = np.where(vec1_len > 1e-12, vec1_len, 1.0)
    cosphi = np.where(vec1_len > 1e-12, np.clip((vec1 @ vec2) / safe, -1.0, 1.0), 1.0)
    vec3 = np.cross(vec2, syn)
    testphi = vec1 @ vec3
    phi = np.where(testphi > 0, np.arccos(cosphi), np.arccos(cosphi) + np.pi)
    phibin = np.clip((phi / 2. / np.pi * NPHIBINS).astype(np.int64), 0, NPHIBINS - 1)
    return costhetabin * NPHIBINS + phibin


def timestep_index(t: np.ndarray, starts: np.ndarray, tmax: float) -> np.ndarray:
    """get_timestep(): index of the timestep [starts[i], starts[i+1]) (the last one ends at tmax) containing t, or -1"""
    idx = np.searchsorted(starts, t, side="right") - 1
    ok = (t >= starts[0]) & (t < tmax)
    return np.where(ok, idx, -1)


def spectrum_and_lightcurve(packets: np.ndarray, ts_starts, ts_widths, tmin: float, tmax: float, vmax: float,
                            nu_min: float = 1e14, nu_max: float = 5e15, dirbin: int = -1):
    """Returns dict(flux[MNUBINS, nts], lower_freq, delta_freq, lum[nts], lumcmf[nts]). dirbin >= 0: the spectrum and light curves
    seen from that direction bin (add_to_spec_res / add_to_lc_res with dirbin, spectrum_lightcurve.cc:545, :689)."""
    starts = np.asarray(ts_starts, dtype=np.float64)
    widths = np.asarray(ts_widths, dtype=np.float64)
    nts_all = len(starts)
    sel = (packets["type"] == TYPE_ESCAPE) & (packets["escape_type"] == TYPE_RPKT)
    p = packets[sel]
    solidanglefactor = 1.0
    if dirbin >= 0:
        p = p[escapedirectionbin(p["dir"]) == dirbin]
        solidanglefactor = float(MABINS)
    dlognu = (np.log(nu_max) - np.log(nu_min)) / MNUBINS
    edges = np.exp(np.log(nu_min) + np.arange(MNUBINS + 1) * dlognu)
    lower = edges[:-1].astype(np.float32)
    delta = (edges[1:] - lower.astype(np.float64)).astype(np.float32)
    t_arrive = p["escape_time"].astype(np.float64) - (p["pos"] * p["dir"]).sum(axis=1) / CLIGHT
    flux = np.zeros((MNUBINS, nts_all))
    lum = np.zeros(nts_all)
    lumcmf = np.zeros(nts_all)
    ok_t = (t_arrive > tmin) & (t_arrive < tmax)
    nts = timestep_index(t_arrive, starts, tmax)
    ok_t &= nts >= 0
    np.add.at(lum, nts[ok_t], p["e_rf"][ok_t] / widths[nts[ok_t]] * solidanglefactor)
    ok = ok_t & (p["nu_rf"] > nu_min) & (p["nu_rf"] < nu_max)
    nnu = np.clip(np.floor((np.log(p["nu_rf"][ok]) - np.log(nu_min)) / dlognu).astype(np.int64), 0, MNUBINS - 1)
    dE = p["e_rf"][ok] / widths[nts[ok]] / delta[nnu].astype(np.float64) / 4.e12 / np.pi / PARSEC / PARSEC * solidanglefactor
    np.add.at(flux, (nnu, nts[ok]), dE)
    inv_gamma = np.sqrt(1. - (vmax * vmax / CLIGHT**2))
    t_cmf = p["escape_time"].astype(np.float64) * inv_gamma
    ok_c = (t_cmf > tmin) & (t_cmf < tmax)
    ntc = timestep_index(t_cmf, starts, tmax)
    ok_c &= ntc >= 0
    np.add.at(lumcmf, ntc[ok_c], p["e_cmf"][ok_c] / widths[ntc[ok_c]] * solidanglefactor / inv_gamma)
    return dict(flux=flux, lower_freq=lower, delta_freq=delta, lum=lum, lumcmf=lumcmf, nescaped=int(len(p)))


# ---- emission / absorption decomposition, Stokes Q / U, gamma outputs and all direction bins (spectrum_lightcurve.cc:168-203,
#      :544-640, exspec.cc:30-130), restated the same way: every output element adds its contributions in packet order (np.add.at)
TYPE_GAMMA = 10
EMTYPE_NOTSET, EMTYPE_FREEFREE = -9999000, -9999999
MEV, H = 1.6021772e-6, 6.6260755e-27
NU_MIN_GAMMA, NU_MAX_GAMMA = 0.05 * MEV / H, 4. * MEV / H  # exspec.cc:61-62


def _grid(nu_min, nu_max):
    dlognu = (np.log(nu_max) - np.log(nu_min)) / MNUBINS
    edges = np.exp(np.log(nu_min) + np.arange(MNUBINS + 1) * dlognu)
    lower = edges[:-1].astype(np.float32)
    return dlognu, lower, (edges[1:] - lower.astype(np.float64)).astype(np.float32)


def max_nions(model) -> int:
    return int(np.max(model["elem_nions"]))


def bf_columns(model) -> np.ndarray:
    """element * max_nions + ion of every bflist entry: the bound-free emission type of (level, target t) is
    -1 - (level_bflist_start[level] + t) (atomic.h:508), for the ionising levels of every ion"""
    mx = max_nions(model)
    cols = np.full(max(int(model["nbfcontinua"]), 1), -1, dtype=np.int64)
    for ui in range(int(model["nions"])):
        el = int(model["ion_element"][ui])
        ion = ui - int(model["elem_uniqueionindexstart"][el])
        l0 = int(model["ion_uniquelevelindexstart"][ui])
        for lv in range(int(model["ion_nlevels_ionising"][ui])):
            for t in range(int(model["level_nphixstargets"][l0 + lv])):
                cols[int(model["level_bflist_start"][l0 + lv]) + t] = el * mx + ion
    return cols


def emission_columns(et: np.ndarray, model, nbfcontinua=None) -> np.ndarray:
    """columnindex_from_emissiontype (spectrum_lightcurve.cc:168-203) of an array of emission types; -1: not counted"""
    et = np.asarray(et, dtype=np.int64)
    nel, mx = int(model["nelements"]), max_nions(model)
    nbf = int(model["nbfcontinua"]) if nbfcontinua is None else nbfcontinua
    nlines = int(model["nlines"])
    out = np.full(et.shape, -1, dtype=np.int64)
    bb = (et >= 0) & (et < nlines)
    out[bb] = model["line_elementindex"][et[bb]].astype(np.int64) * mx + model["line_ionindex"][et[bb]]
    out[et == EMTYPE_FREEFREE] = 2 * nel * mx
    bf = (et < 0) & (et != EMTYPE_FREEFREE) & (et != EMTYPE_NOTSET)
    if nbf == 0:
        out[bf] = 2 * nel * mx
    else:
        idx = -1 - et
        ok = bf & (idx < nbf)
        cols = bf_columns(model)[idx[ok]]
        out[ok] = np.where(cols >= 0, nel * mx + cols, -1)  # an entry that no level's target fills: not counted
    return out


def _escaped_rpkts(packets, dirbin):
    sel = (packets["type"] == TYPE_ESCAPE) & (packets["escape_type"] == TYPE_RPKT)
    p = packets[sel]
    if dirbin >= 0:
        return p[escapedirectionbin(p["dir"]) == dirbin], float(MABINS)
    return p, 1.0


def stokes_and_emission_absorption(packets: np.ndarray, ts_starts, ts_widths, tmin: float, tmax: float, model,
                                   nu_min: float = 1e14, nu_max: float = 5e15, dirbin: int = -1, emission_absorption: bool = True,
                                   stokes: bool = True, nbfcontinua=None) -> dict:
    """add_to_spec_res (:544-640) beyond the flux: flux_q / flux_u [MNUBINS, nts] (stokes); emission(_q, _u), trueemission
    [MNUBINS, nts, proccount] and absorption(_q, _u) [MNUBINS, nts, nelements * max_nions] (emission_absorption)."""
    starts = np.asarray(ts_starts, dtype=np.float64)
    widths = np.asarray(ts_widths, dtype=np.float64)
    T = len(starts)
    nel, mx = int(model["nelements"]), max_nions(model)
    P, A = 2 * nel * mx + 1, nel * mx
    p, saf = _escaped_rpkts(packets, dirbin)
    dlognu, lower, delta = _grid(nu_min, nu_max)
    t_arrive = p["escape_time"].astype(np.float64) - (p["pos"] * p["dir"]).sum(axis=1) / CLIGHT
    nts = timestep_index(t_arrive, starts, tmax)
    ok = (t_arrive > tmin) & (t_arrive < tmax) & (nts >= 0) & (p["nu_rf"] > nu_min) & (p["nu_rf"] < nu_max)
    p, nts = p[ok], nts[ok]
    nnu = np.clip(np.floor((np.log(p["nu_rf"]) - np.log(nu_min)) / dlognu).astype(np.int64), 0, MNUBINS - 1)
    dE = p["e_rf"] / widths[nts] / delta[nnu].astype(np.float64) / 4.e12 / np.pi / PARSEC / PARSEC * saf
    out = {}
    if stokes:
        for k, f in (("q", "stokes_q"), ("u", "stokes_u")):
            a = np.zeros((MNUBINS, T))
            np.add.at(a, (nnu, nts), p[f] * dE)
            out["flux_" + k] = a
    if not emission_absorption:
        return out
    comps = [("", None)] + ([("_q", "stokes_q"), ("_u", "stokes_u")] if stokes else [])
    true_col = emission_columns(p["trueemissiontype"], model, nbfcontinua)
    t = true_col >= 0
    a = np.zeros((MNUBINS, T, P))
    np.add.at(a, (nnu[t], nts[t], true_col[t]), dE[t])
    out["trueemission"] = a
    col = emission_columns(p["emissiontype"], model, nbfcontinua)
    m = col >= 0
    for suffix, f in comps:
        a = np.zeros((MNUBINS, T, P))
        np.add.at(a, (nnu[m], nts[m], col[m]), dE[m] if f is None else p[f][m] * dE[m])
        out["emission" + suffix] = a
    at = p["absorptiontype"].astype(np.int64)
    b = (at >= 0) & (at < int(model["nlines"])) & (p["absorptionfreq"] > nu_min) & (p["absorptionfreq"] < nu_max)
    pb, ntb, atb = p[b], nts[b], at[b]
    nnu_abs = np.clip(np.floor((np.log(pb["absorptionfreq"]) - np.log(nu_min)) / dlognu).astype(np.int64), 0, MNUBINS - 1)
    acol = model["line_elementindex"][atb].astype(np.int64) * mx + model["line_ionindex"][atb]
    dEa = pb["e_rf"] / widths[ntb] / delta[nnu_abs].astype(np.float64) / 4.e12 / np.pi / PARSEC / PARSEC * saf
    for suffix, f in comps:
        a = np.zeros((MNUBINS, T, A))
        np.add.at(a, (nnu_abs, ntb, acol), dEa if f is None else pb[f] * dEa)
        out["absorption" + suffix] = a
    return out


def gamma_spectrum_and_lightcurve(packets: np.ndarray, ts_starts, ts_widths, tmin: float, tmax: float, vmax: float) -> dict:
    """The escaped gamma packets (exspec.cc:80-86): gamma_lum, gamma_lumcmf [nts] and gamma_flux [MNUBINS, nts] over
    0.05 .. 4 MeV, angle-averaged"""
    g = packets[(packets["type"] == TYPE_ESCAPE) & (packets["escape_type"] == TYPE_GAMMA)].copy()
    g["escape_type"] = TYPE_RPKT  # the same rules on the gamma frequency grid
    r = spectrum_and_lightcurve(g, ts_starts, ts_widths, tmin, tmax, vmax, NU_MIN_GAMMA, NU_MAX_GAMMA)
    return dict(gamma_lum=r["lum"], gamma_lumcmf=r["lumcmf"], gamma_flux=r["flux"], gamma_lower_freq=r["lower_freq"],
                gamma_delta_freq=r["delta_freq"], nescaped_gamma=r["nescaped"])


def all_dirbins(fn, *args, **kwargs) -> dict:
    """fn(..., dirbin=b) for the angle average and every direction bin, stacked along a leading axis of 1 + MABINS
    (slot 0: the angle average, slot s: direction bin s - 1); array outputs only"""
    res = [fn(*args, dirbin=b, **kwargs) for b in range(-1, MABINS)]
    return {k: np.stack([r[k] for r in res]) for k, v in res[0].items() if isinstance(v, np.ndarray) and k not in
            ("lower_freq", "delta_freq")}
