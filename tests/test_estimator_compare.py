"""CPU tests of the estimator comparison itself (tests/parity.py compare_estimators) on real oracle outputs: the per-entry bar
rejects the errors that the max-relative bar lets through (a dropped or doubled flush of a dim cell's sums, a small relative
error in a dim entry), and it still accepts the same terms summed in another order.

Cases: w7 atomic data on a 20^3 Cartesian grid, classic options (ffheatingestimator, bfheatingestimator span many decades); and
the small atomic data under the nltenebular options on 8^3 (bfrate_raw, radfieldbin_J / _nuJ).
"""
import copy
import os
import re

import numpy as np
import pytest

import parity
from artis_amd import abi, synth

RTOL = 1e-9  # EST_RTOL of the GPU parity tests
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "w7_20cubed_classic": dict(build=dict(preset="w7", ncoord=20), npk=20000, options="classic"),
    "small_8cubed_nltenebular": dict(build=dict(preset="small", ncoord=8, options="nltenebular", nts=13), npk=8000,
                                     options="nltenebular"),
}


def old_check(got, want, rtol=RTOL):
    """The bar compare_estimators held before the per-entry checks: each array to rtol of its own largest entry."""
    for k, a in got.arrays().items():
        b = want.arrays()[k]
        if np.abs(a - b).max() / max(np.abs(b).max(), 1e-300) > rtol:
            return False
    return True


def new_check(got, want, rtol=RTOL):
    try:
        parity.compare_estimators(got, want, rtol, "perturbed")
    except AssertionError as e:
        return str(e)
    return None


@pytest.fixture(scope="module")
def runs(oracle):
    """{case: (oracle estimators of one serial call, the same packets' estimators from 7 forked slices added up)}"""
    out = {}
    for name, c in CASES.items():
        model, cs, ts, aux = synth.build(**c["build"])
        pk0 = synth.make_packets(model, aux, c["npk"], kpkt_fraction=0.1, gamma_fraction=0.1)
        pa, ea = pk0.copy(), abi.estimators_for(model, c["options"])
        oracle.update_packets(model, cs, ts, pa, ea, preset=c["options"])
        pb, eb = pk0.copy(), abi.estimators_for(model, c["options"])
        parity.oracle_parallel(model, cs, ts, pb, eb, preset=c["options"], nproc=7)
        parity.compare_packets(pb, pa, 0.0, name)  # the same packets: only the grouping of the sums differs
        out[name] = (ea, eb)
    return out


def _copy(est):
    c = copy.copy(est)
    for k, a in est.arrays().items():
        setattr(c, k, a.copy())
    c.stats = est.stats.copy()
    return c


def _dim_arrays(est, below):
    """(array name, flat index) of the non-zero entries below `below` x the array's max, per float array"""
    out = []
    for k, a in est.arrays().items():
        if k in parity.NOT_PER_CELL or not np.issubdtype(a.dtype, np.floating):
            continue
        nz = np.nonzero((a != 0) & (np.abs(a) < below * np.abs(a).max()))[0]
        if len(nz):
            out.append((k, nz))
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_against_itself_passes(runs, case):
    ea, _ = runs[case]
    worst = parity.compare_estimators(_copy(ea), ea, RTOL, case)
    assert all(w == 0.0 for w in worst.values())


@pytest.mark.parametrize("case", sorted(CASES))
def test_reordered_summation_passes(runs, case):
    """The same terms added in another grouping (7 slices of the population, each summed on its own, then added): not
    bit-identical, and within the per-entry bar -- the bar does not demand bitwise equality."""
    ea, eb = runs[case]
    assert any(not np.array_equal(a, ea.arrays()[k]) for k, a in eb.arrays().items()), "the regrouping changed no sum"
    worst = parity.compare_estimators(eb, ea, RTOL, case)
    assert max(worst.values()) < 1e-13, worst


@pytest.mark.parametrize("case", sorted(CASES))
def test_dim_entries_are_real(runs, case):
    """The cases hold what the perturbations need: entries far below their array's max in the arrays named"""
    ea, _ = runs[case]
    dim = dict(_dim_arrays(ea, 1e-6))
    want = ("ffheatingestimator", "bfheatingestimator") if "classic" in case else ("bfrate_raw",)
    for k in want:
        assert k in dim and len(dim[k]) > 10, (k, sorted(dim))
    if "nltenebular" in case:
        assert np.count_nonzero(ea.radfieldbin_J) > 1000 and np.count_nonzero(ea.bfrate_raw) > 1000


@pytest.mark.parametrize("case", sorted(CASES))
def test_zeroed_smallest_entry_is_rejected(runs, case):
    """A lost flush of the dimmest sum: its array's smallest non-zero entry set to zero"""
    ea, _ = runs[case]
    n = 0
    for k, a in ea.arrays().items():
        if k in parity.NOT_PER_CELL or not np.issubdtype(a.dtype, np.floating) or np.count_nonzero(a) < 2:
            continue
        nz = np.nonzero(a)[0]
        i = nz[np.argmin(np.abs(a[nz]))]
        if abs(a[i]) > RTOL * np.abs(a).max():
            continue  # (the old bar catches this one itself)
        got = _copy(ea)
        got.arrays()[k][i] = 0.0
        assert old_check(got, ea), k
        msg = new_check(got, ea)
        assert msg is not None and k in msg and "support" in msg, (k, msg)
        n += 1
    assert n >= 1


@pytest.mark.parametrize("case", sorted(CASES))
def test_small_relative_error_in_dim_entry_is_rejected(runs, case):
    """One entry below 1e-6 of its array's max off by 1e-6 of its own value, in every array that has such an entry"""
    ea, _ = runs[case]
    dim = _dim_arrays(ea, 1e-6)
    assert dim
    for k, idx in dim:
        got = _copy(ea)
        i = idx[len(idx) // 2]
        got.arrays()[k][i] *= 1 + 1e-6
        assert old_check(got, ea), k
        msg = new_check(got, ea)
        assert msg is not None and f"{k}[{i}]" in msg and "per-entry" in msg, (k, msg)
        if k not in parity.NOT_PER_CELL:
            stride = len(got.arrays()[k]) // len(ea.J)
            assert f"cell {i // stride}," in msg, msg


@pytest.mark.parametrize("case,array", [("w7_20cubed_classic", "J"), ("small_8cubed_nltenebular", "radfieldbin_J")])
def test_misplaced_dim_cell_contribution_is_rejected(runs, case, array):
    """A contribution of a dim cell added to its dim neighbour's record instead (a flush to the wrong cell): the total is unchanged
    and the moved amount is below 1e-9 of the array's max (both entries below 1e-2 of it; the nltenebular 8^3 grid has no dim
    cells in J, so a radiation-field bin there)"""
    ea, _ = runs[case]
    a = ea.arrays()[array]
    stride = len(a) // len(ea.J)
    dim = (a > 0) & (a < 1e-2 * a.max())
    pairs = [(i, i + stride) for i in np.nonzero(dim)[0] if i + stride < len(a) and dim[i + stride]]
    assert pairs, "no two neighbouring dim cells"
    i, j = min(pairs, key=lambda p: a[p[0]] + a[p[1]])
    moved = min(a[i], 0.9 * RTOL * a.max())
    got = _copy(ea)
    got.arrays()[array][i] -= moved
    got.arrays()[array][j] += moved
    assert old_check(got, ea)
    msg = new_check(got, ea)
    assert msg is not None and f"estimator {array}[" in msg and "per-entry" in msg, msg


def test_signed_stokes_and_integer_arrays():
    """Stokes Q / U of the virtual-packet spectra are bounded by the I of their bin (not skipped for being signed); an integer
    array must be equal; a signed array without a rule is refused"""
    n = 4
    want = abi.Estimators(n, 1, vpkt_shape=(1, 0))
    want.J[:] = 1.0
    v = want.vspecpol.reshape(-1, 3)
    rng = np.random.default_rng(3)
    v[:50, 0] = 10.0 ** rng.uniform(-12, 0, 50)           # I, many decades
    v[:50, 1] = v[:50, 0] * rng.uniform(-1, 1, 50)         # Q, U: |q|, |u| <= I
    v[:50, 2] = v[:50, 0] * rng.uniform(-1, 1, 50)
    v[3, 1] = 0.0                                          # a Q that happens to be zero where I is not
    assert parity.compare_estimators(_copy(want), want, RTOL) is not None
    i = int(np.argmin(v[:50, 0]))
    got = _copy(want)
    got.vspecpol.reshape(-1, 3)[i, 1] += 0.5 * RTOL * v[i, 0]  # within elem_rtol x I of its bin: accepted
    got.vspecpol.reshape(-1, 3)[3, 1] = 1e-3 * RTOL * v[3, 0]  # Q leaves zero, by a hair of I: accepted
    parity.compare_estimators(got, want, RTOL)
    got.vspecpol.reshape(-1, 3)[i, 2] += 3 * RTOL * v[i, 0]    # U beyond it, still far below 1e-9 of the array's max
    assert old_check(got, want)
    assert "vspecpol" in new_check(got, want)
    got = _copy(want)
    got.vspecpol.reshape(-1, 3)[60] = [1e-20, 0.0, 0.0]       # flux in a bin the oracle has none in
    assert old_check(got, want) and "support" in new_check(got, want)
    # integer arrays: equal
    w2 = abi.Estimators(2, 1, nbfcontinua=1, ndetailedlines=2)
    w2.Jb_lu_contribcount[:] = [5_000_000_000, 0, 7, 1]
    g2 = _copy(w2)
    g2.Jb_lu_contribcount[2] = 8
    assert old_check(g2, w2) and "integer" in new_check(g2, w2)
    # a signed array that is not a Stokes component has no rule
    w3 = abi.Estimators(n, 1)
    w3.J[:] = [1.0, -1e-3, 2.0, 3.0]
    assert "negative" in new_check(_copy(w3), w3)


def test_estimator_form_names_match_header():
    """abi.EST_FORMS mirrors the ARTIS_AMD_EST_* masks of include/artis_amd.h (artis_amd_last_estimator_forms)"""
    hdr = open(os.path.join(ROOT, "include", "artis_amd.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ARTIS_AMD_EST_(\w+)\s+(\d+)", hdr)}
    assert defs == abi.EST_FORMS
    assert all(v & (v - 1) == 0 for v in defs.values()) and len(set(defs.values())) == len(defs)
