"""Shared comparison helpers for the parity tests (engine or emulated kernel bodies vs the CPU oracle)."""
from __future__ import annotations

import numpy as np

from artis_amd import abi

# Reference-defined counters must match exactly; so must the step counters this project adds.
EXACT_STATS = list(range(abi.STAT_COUNT)) + [abi.STAT_X_RPKT_STEPS, abi.STAT_X_KPKT_STEPS, abi.STAT_X_LINES_VISITED,
                                            abi.STAT_X_MA_JUMPS,
                                            # virtual packets created / escaped after an r-packet, k-packet, macro-atom (VPKT_ON builds)
                                            *range(abi.STAT_X_VPKT_CREATED, abi.STAT_X_VPKT_CREATED + 4)]


STOKES_ABS_FLOOR = 1e-12  # above the largest absolute q / u difference ever measured against the oracle (1.6e-13)


def compare_packets(got: np.ndarray, want: np.ndarray, rtol: float, what: str = "") -> dict:
    """Integer fields (type, cell, line indices, emission/absorption types, scatter counts) and the RNG state
    must be identical; floating-point fields within rtol (0.0 = bit-exact), vectors relative to their length."""
    assert len(got) == len(want)
    rep = {}
    for f in abi.PACKET_INT_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{what}: integer field {f} differs for {len(bad)} packets, first {bad[:5]}: {got[f][bad[:5]]} vs {want[f][bad[:5]]}"
    assert np.array_equal(got["rngstate"], want["rngstate"]), f"{what}: RNG state differs (a different number of draws was made)"
    worst = 0.0
    for f in abi.PACKET_FLOAT_FIELDS:
        a = np.asarray(got[f], dtype=np.float64)
        b = np.asarray(want[f], dtype=np.float64)
        both_nan = np.isnan(a) & np.isnan(b)
        if rtol == 0.0:
            same = (a == b) | both_nan
            assert same.all(), f"{what}: float field {f} not bit-identical for {np.count_nonzero(~same)} values"
        else:
            if a.ndim == 2:  # 3-vectors (pos, dir, em_pos, trueem_pos): error relative to the length of the vector,
                # not to each component (a component that happens to be ~0 carries the absolute rounding of the others)
                denom = np.broadcast_to(np.sqrt(np.nansum(b * b, axis=1))[:, None], a.shape).copy()
            else:
                denom = np.maximum(np.abs(a), np.abs(b))
            denom[~(denom > 0)] = 1.0
            rel = np.abs(a - b) / denom
            rel[both_nan] = 0.0
            if f in ("stokes_q", "stokes_u"):
                # q, u are differences of O(1) terms of the normalised Stokes vector (vectors.h:266-370), so a value near zero carries the
                # ABSOLUTE rounding of those terms: every value has to meet the relative bar OR lie within STOKES_ABS_FLOOR of the
                # oracle's. (Round 4, 2e6 packets: one packet with q = -3.2e-7 differed by 3.7e-16 = 1.2e-9 of |q|; the largest absolute
                # difference of all packets was 1.6e-13: profiles/r04/stress_parity_2e6.txt. Round 4 measured q, u against |(1, q, u)|
                # instead, which turned the bar into an absolute 1e-9 for every packet)
                rel[np.abs(a - b) <= STOKES_ABS_FLOOR] = 0.0
            assert not np.isnan(rel).any(), f"{what}: NaN mismatch in {f}"
            worst = max(worst, float(rel.max()))
            assert rel.max() <= rtol, f"{what}: float field {f} rel diff {rel.max():.3e} > {rtol}"
    rep["worst_rel"] = worst
    return rep


# estimator arrays that are not [cell][...]: the per-timestep scalar sums and the virtual-packet spectra / velocity-grid map
NOT_PER_CELL = ("scalars", "vspecpol", "vgrid_flux")
# arrays of Stokes triples {I, Q, U} in their last axis (include/artis_amd.h artis_estimators: vspecpol[..][nubin].{I, Q, U},
# vgrid[..][obsdir].{I, Q, U}; physics.h add_to_vspecpol / add_to_vpkt_grid): I is a sum of non-negative terms, Q and U are signed
STOKES_ARRAYS = ("vspecpol", "vgrid_flux")


def _est_fail(what, k, idx, a, b, stride, why):
    scale = max(float(np.abs(b).max()), 1e-300)
    cell = f"cell {idx // stride}, " if stride else ""
    return (f"{what}: estimator {k}[{idx}] ({cell}got {a[idx]!r}, oracle {b[idx]!r}, "
            f"{abs(float(b[idx])) / scale:.3e} of the array's max): {why}")


def compare_estimators(got: abi.Estimators, want: abi.Estimators, rtol: float, what: str = "",
                       elem_rtol: float | None = None) -> dict:
    """Estimators are sums of many terms; the GPU adds them with atomics in arbitrary order (float sums are not associative).
    Two bars, both must hold for every array:
    - max-relative: max |got - want| <= rtol x the largest |want| of the array;
    - per entry (elem_rtol, default rtol): every array is a sum of non-negative terms (asserted on the oracle's side), so an
      entry is zero on one side exactly when it is zero on the other, and |got - want| <= elem_rtol x |want| entry by entry --
      a dim cell's sums are held to their own size, not to the brightest cell's. Integer arrays (Jb_lu_contribcount) are
      equal. The Stokes Q and U of the virtual-packet spectra are signed: |dQ|, |dU| <= (elem_rtol + STOKES_ABS_FLOOR) x the
      oracle's I of the same bin (each term's q, u is its I-term times a normalised q, u in [-1, 1] that carries up to
      STOKES_ABS_FLOOR of absolute rounding: compare_packets).
    Returns {array: worst per-entry relative difference}."""
    elem_rtol = rtol if elem_rtol is None else elem_rtol
    ncell = len(want.J)
    worst = {}
    for k, a in got.arrays().items():
        b = want.arrays()[k]
        assert a.shape == b.shape, f"{what}: estimator {k} shape {a.shape} vs {b.shape}"
        scale = max(np.abs(b).max(), 1e-300)
        err = np.abs(a - b).max() / scale
        assert err <= rtol, f"{what}: estimator {k} differs by {err:.3e} (rel. to max) > {rtol}"
        stride = (len(b) // ncell) if (k not in NOT_PER_CELL and len(b) >= ncell and len(b) % ncell == 0) else 0
        if np.issubdtype(b.dtype, np.integer):
            bad = np.nonzero(a != b)[0]
            assert len(bad) == 0, _est_fail(what, k, bad[0], a, b, stride, f"integer estimator differs at {len(bad)} entries")
            worst[k] = 0.0
            continue
        a = np.asarray(a, dtype=np.float64)
        b = np.asarray(b, dtype=np.float64)
        assert np.isfinite(b).all(), f"{what}: oracle estimator {k} is not finite"
        bad = np.nonzero(~np.isfinite(a))[0]
        assert len(bad) == 0, _est_fail(what, k, bad[0], a, b, stride, "not finite")
        diff = np.abs(a - b)
        if k in STOKES_ARRAYS and len(b) % 3 == 0:  # (a size-1 placeholder when the build has no such output)
            I, Ig = b.reshape(-1, 3)[:, 0], a.reshape(-1, 3)[:, 0]
            assert (I >= 0).all(), f"{what}: oracle Stokes I of {k} has negative entries"
            bound = np.repeat((elem_rtol + STOKES_ABS_FLOOR) * I, 3)
            bound[0::3] = elem_rtol * I
            signed = np.zeros(len(b), dtype=bool)
            signed[1::3] = signed[2::3] = True
            # support: a bin with no flux in I has no Q, U either; I itself is zero on one side exactly when on the other
            zero_ref = np.repeat(I == 0, 3)
            bad = np.nonzero(zero_ref & (a != 0) | np.repeat((Ig == 0) != (I == 0), 3))[0]
            assert len(bad) == 0, _est_fail(what, k, bad[0], a, b, 0, f"support differs at {len(bad)} entries (bin of zero I)")
            denom = np.where(signed, np.repeat(I, 3), np.abs(b))
        else:
            neg = np.nonzero(b < 0)[0]
            assert len(neg) == 0, _est_fail(what, k, neg[0], a, b, stride, "the oracle's entry is negative: a signed estimator needs a rule of its own")
            bad = np.nonzero((a == 0) != (b == 0))[0]
            assert len(bad) == 0, _est_fail(what, k, bad[0], a, b, stride, f"support differs at {len(bad)} entries")
            bound = elem_rtol * b
            denom = b
        over = np.nonzero(diff > bound)[0]
        if len(over):
            i = over[np.argmax(diff[over] / np.maximum(denom[over], 1e-300))]
            raise AssertionError(_est_fail(what, k, i, a, b, stride,
                                           f"per-entry difference {diff[i] / max(denom[i], 1e-300):.3e} of its own value > {elem_rtol} "
                                           f"at {len(over)} entries"))
        nz = denom > 0
        worst[k] = float((diff[nz] / denom[nz]).max()) if nz.any() else 0.0
    return worst


UPDATECELL = abi.STAT_NAMES.index("UPDATECELL")
UPSCATTER = abi.STAT_NAMES.index("UPSCATTER")
DOWNSCATTER = abi.STAT_NAMES.index("DOWNSCATTER")


def compare_stats(got: abi.Estimators, want: abi.Estimators, what: str = "", same_libm: bool = True) -> None:
    """Event counters (stats.h:13 of the reference, plus this project's step counters) must be identical.
    UPDATECELL is skipped: the engine fills the cache of every cell up front, the oracle on first use.
    With different math libraries (GPU vs glibc) UPSCATTER and DOWNSCATTER are compared as a sum: the
    reference classifies a line scattering by `oldnucmf < nu_cmf` (macroatom.cc:232), and for a resonance
    scattering the two frequencies are equal to the last bit or two, so the split is not a property of the
    algorithm but of the exp/log rounding of the platform."""
    for i in EXACT_STATS:
        if i == UPDATECELL:
            continue
        if not same_libm and i in (UPSCATTER, DOWNSCATTER):
            continue
        assert got.stats[i] == want.stats[i], f"{what}: event counter {abi.STAT_NAMES[i]}: {got.stats[i]} vs {want.stats[i]}"
    assert got.stats[UPSCATTER] + got.stats[DOWNSCATTER] == want.stats[UPSCATTER] + want.stats[DOWNSCATTER], what


def _oracle_init(md, cd, tsargs, preset):
    from oracle import oracle_py

    oracle_py.lib(preset)
    _oracle_slice.shared = (abi.Model(md), abi.CellState(cd), abi.Timestep(*tsargs), preset)


def _oracle_slice(sub):
    from oracle import oracle_py

    model, cs, ts, preset = _oracle_slice.shared
    est = abi.estimators_for(model, preset)
    oracle_py.update_packets(model, cs, ts, sub, est, preset=preset)
    return sub, est.arrays(), np.array(est.stats)


def oracle_parallel(model, cs, ts, pk, est: abi.Estimators, preset: str = "classic", nproc: int = 0) -> None:
    """The CPU oracle on slices of the population in worker processes (packets are independent: per-packet generator, per-packet
    opacity cache), results written back into pk and added into est. Event counters add exactly; estimators are float sums whose
    order differs from a single call, which the comparison tolerance covers.
    The workers are SPAWNED, fresh interpreters that are handed the model and their slice: never forked, so that none inherits
    the device of a process that has already opened the GPU (an earlier module of a `-m gpu` run may have)."""
    import multiprocessing as mp
    import os

    from oracle import oracle_py

    oracle_py.lib(preset)  # built (if its sources are newer) here, not by every worker at once
    nproc = nproc or min(os.cpu_count() or 1, 16)
    n = len(pk)
    bounds = [(n * i // nproc, n * (i + 1) // nproc) for i in range(nproc)]
    t = ts.c
    init = (model.d, cs.d, (t.nts, t.start, t.width, t.mid, t.max_path_step), preset)
    with mp.get_context("spawn").Pool(nproc, initializer=_oracle_init, initargs=init) as pool:
        res = pool.map(_oracle_slice, [pk[lo:hi].copy() for lo, hi in bounds])
    for (lo, hi), (sub, arrs, stats) in zip(bounds, res):
        pk[lo:hi] = sub
        for k, a in est.arrays().items():
            a += arrs[k]
        est.stats[:] = np.asarray(est.stats) + stats
