"""The rules of the decay and abundance update (artis_amd/csrc/decay_update.h) in their x86 build (tests/decay_host): the Bateman sum
against known answers and against 80-digit arithmetic (tests/golden/bateman_reference.json), the per-cell bodies against a
sequential float64 restatement of decay.cc:1204-1276 and update_grid.cc:718 written here, conservation of mass, the validator and the
row builder. No GPU."""
import json
import os

import numpy as np
import pytest

import decay_common as dc
from artis_amd import abi, synth

DAY, EPS = dc.DAY, dc.EPS
GOLDEN = os.path.join(dc.HERE, "golden", "bateman_reference.json")
GRIDS = {"3d": abi.GRID_CARTESIAN3D, "1d": abi.GRID_SPHERICAL1D}


@pytest.fixture(scope="module")
def nets():
    return {k: synth.decay_network(k) for k in ("small", "small_nohe4")}


@pytest.fixture(scope="module")
def setups(nets):
    """(grid, network) -> (model, decay model, HostDecay)"""
    out = {}
    for g, gt in GRIDS.items():
        model, cs, ts, aux = dc.grid(gt)
        for k, net in nets.items():
            dm = synth.decay_model(model, cs, aux, net, t_model=dc.T_MODEL)
            out[(g, k)] = (model, dm, dc.HostDecay(dm, model))
    return out


def test_network_is_the_one_the_tests_need(nets, setups):
    net = nets["small"]
    L = np.diff(net["path_start"])
    assert 28 <= len(net["nuc_z"]) <= 34 and 160 <= len(L) <= 200 and L.max() == 15
    life = net["nuc_meanlife"]
    assert life.max() > 1e17 and 0 < life[life > 0].min() < 1e-3
    ends_tops = [(net["path_nucindex"][net["path_start"][p]], net["path_nucindex"][net["path_start"][p + 1] - 1]) for p in range(len(L))]
    assert len(set(ends_tops)) < len(ends_tops)  # two paths share top and end
    model, dm, host = setups[("3d", "small")]
    assert int(model["npts_nonempty"]) % 64 != 0 and int(setups[("1d", "small")][0]["npts_nonempty"]) == 5
    per_el = [int((net["nuc_z"] == z).sum()) for z in model["elem_anumber"]]
    assert sum(k >= 3 for k in per_el) >= 2 and 0 in per_el
    assert (~np.isin(net["nuc_z"], model["elem_anumber"])).any()
    el0 = per_el.index(0)
    assert (dm["elem_untrackedstable_initmassfrac"][:, el0] == 0).sum() == 1
    assert host.he4 == len(net["nuc_z"]) - 1 and setups[("3d", "small_nohe4")][2].he4 == -1


def test_known_answers():
    """the three checks of the reference's own unit test of the Bateman sum without the expansion factor, at their tolerances"""
    la, lb, t, n0 = 1.0 / (8.80 * DAY), 1.0 / (113.7 * DAY), 30.0 * DAY, 2.5

    def close(got, want, tol):
        assert abs(got - want) <= tol * abs(want), (got, want)

    close(n0 * dc.decaychain([la], t)[0], n0 * np.exp(-la * t), 1e-14)
    close(n0 * dc.decaychain([la, lb], t)[0], n0 * la / (lb - la) * (np.exp(-la * t) - np.exp(-lb * t)), 1e-12)
    close(n0 * dc.decaychain([la, 0.0], 1000.0 * 8.80 * DAY)[0], n0, 1e-12)


def test_bateman_sums_against_80_digit_arithmetic(nets):
    """Every path of the small network at the six times: |harness - exact| <= 4 (L + x_dom) 2^-52 scale, L the path's length, scale =
    lambdaproduct x the largest |term|, x_dom = lambda t of that term (the exp's argument carries x eps). The alpha-terminated paths
    also with the last decay constant zeroed (the He4 coefficient's sum)."""
    net = nets["small"]
    ref = json.load(open(GOLDEN))
    assert tuple(ref["times_days"]) == dc.TIMES_DAYS and len(ref["paths"]) == len(net["path_start"]) - 1
    worst, nzero_scale = 0.0, 0
    for p, e in enumerate(ref["paths"]):
        lam = dc.path_lambdas(net, p)
        assert [float(x).hex() for x in lam] == e["lambdas_hex"], f"path {p}: the golden file is of another network (make_bateman_golden.py)"
        variants = [(lam, e["exact"])]
        if e["exact_sink"] is not None:
            variants.append((np.concatenate([lam[:-1], [0.0]]), e["exact_sink"]))
        for lams, exact in variants:
            for days, ex in zip(dc.TIMES_DAYS, exact):
                got, scale, x_dom = dc.decaychain(lams, days * DAY)
                if scale < np.finfo(np.float64).tiny:  # underflowed: no relative precision left, the rule gives 0
                    nzero_scale += 1
                    assert got == 0.0, (p, days)
                    continue
                bar = 4 * (len(lams) + x_dom) * EPS * scale
                assert abs(got - float(ex)) <= bar, (p, days, got, ex, bar)
                worst = max(worst, abs(got - float(ex)) / bar)
    print(f"worst |harness - exact| / bar = {worst:.3f}; {nzero_scale} sums with an underflowed scale")


def restate(dm, he4, co, t_mid, tmin, Z, reverse=False):
    """decay.cc:1204-1276 and update_grid.cc:718 with sequential float64 operations (vectors over the cells; numpy's elementwise
    products and sums are single IEEE operations, never fused)"""
    X = np.asarray(dm["initnucmassfrac"], np.float32).astype(np.float64)
    n, nn = X.shape
    start, idx = dm["path_start"], dm["path_nucindex"]
    mf = co["survivingfrac"][None, :] * X
    order = range(len(start) - 1)
    for p in (reversed(order) if reverse else order):
        top, end = idx[start[p]], idx[start[p + 1] - 1]
        mf[:, end] = mf[:, end] + co["endnuc_coeff"][p] * X[:, top]
        if he4 >= 0:
            mf[:, he4] = mf[:, he4] + co["he4_coeff"][p] * X[:, top]
    ne = len(Z)
    s1, s2 = np.zeros((n, ne)), np.zeros((n, ne))
    for nuc in range(nn):
        el = [i for i, z in enumerate(Z) if z == dm["nuc_z"][nuc]]
        if el:
            s1[:, el[0]] = s1[:, el[0]] + mf[:, nuc]
            s2[:, el[0]] = s2[:, el[0]] + mf[:, nuc] / (float(dm["nuc_a"][nuc]) * synth.MH)
    other = np.asarray(dm["elem_untrackedstable_initmassfrac"], np.float32).astype(np.float64).reshape(n, ne)
    stable = np.asarray(dm["elem_initstablemeannucmass"], np.float32)
    iso = s1 + other
    iso_on = s2 + other / stable.astype(np.float64)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        mw = (iso / iso_on).astype(np.float32)
    mw = np.where(np.isfinite(mw) & (mw > 0), mw, stable[None, :]).astype(np.float32)
    r = t_mid / tmin
    rho = (np.asarray(dm["rho_tmin"], np.float32).astype(np.float64) / (r * r * r)).astype(np.float32)
    return dict(nuc_massfracs=mf, elem_massfracs=iso.astype(np.float32), elem_meanweight=mw, rho=rho)


@pytest.mark.parametrize("netkind", ["small", "small_nohe4"])
@pytest.mark.parametrize("g", list(GRIDS))
@pytest.mark.parametrize("days", [20.0, 300.0])
def test_cell_bodies_bit_identical_to_a_sequential_restatement(setups, g, netkind, days):
    model, dm, host = setups[(g, netkind)]
    t_mid = dc.T_MODEL + days * DAY
    co = host.coeffs(t_mid)
    got = host.cells(t_mid, co)
    want = restate(dm, host.he4, co, t_mid, float(model["tmin"]), [int(z) for z in model["elem_anumber"]])
    for k in ("nuc_massfracs", "elem_massfracs", "elem_meanweight", "rho"):
        assert got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))
    # the mean-weight fallback was taken where the element has nothing
    el0 = [int((dm["nuc_z"] == z).sum()) for z in model["elem_anumber"]].index(0)
    c0 = int(np.nonzero(dm["elem_untrackedstable_initmassfrac"][:, el0] == 0)[0][0])
    assert got["elem_massfracs"][c0, el0] == 0 and got["elem_meanweight"][c0, el0] == dm["elem_initstablemeannucmass"][el0]
    # the identity is about order: the same sums taken in reversed path order differ somewhere
    rev = restate(dm, host.he4, co, t_mid, float(model["tmin"]), [int(z) for z in model["elem_anumber"]], reverse=True)
    rows = np.diff(host.rows()["row_start"])
    assert rows.max() > 1 and (rev["nuc_massfracs"] != want["nuc_massfracs"]).any()


@pytest.mark.parametrize("g", list(GRIDS))
def test_mass_is_conserved(setups, nets, g):
    """With He4 in the network every decay keeps the mass number: per cell the nuclides' mass fractions add up to the initial ones.
    What the arithmetic may lose: every path's coefficient is branchproduct x Bateman sum x A_end / A_top with the sum within
    4 (L + x) eps scale of exact (the bar of the test above, which also covers a sum the clamp set to 0, since the clamp acts only
    below L eps x the largest term), so the path's contribution is off by at most that x branchproduct x X_top x A_end / A_top; the
    products, the surviving fractions and the additions of at most nnuclides + npaths numbers that add up to about the cell's total
    (<= 1) each round once: nnuclides eps covers them generously for totals of order 1e-1."""
    net = nets["small"]
    model, dm, host = setups[(g, "small")]
    X = np.asarray(dm["initnucmassfrac"], np.float64)
    A = net["nuc_a"].astype(np.float64)
    L = np.diff(net["path_start"]).astype(np.float64)
    top = net["path_nucindex"][net["path_start"][:-1]]
    end = net["path_nucindex"][net["path_start"][1:] - 1]
    worst = 0.0
    for days in dc.TIMES_DAYS:
        t_mid = dc.T_MODEL + days * DAY
        co = host.coeffs(t_mid)
        out = host.cells(t_mid, co)
        w = 4 * (L + co["path_x_dom"]) * EPS * co["path_scale"] * net["path_branchproduct"] * A[end] / A[top]
        bound = X[:, top] @ w + len(A) * EPS
        diff = np.abs(out["nuc_massfracs"].sum(axis=1) - X.sum(axis=1))
        assert (diff <= bound).all(), (days, float((diff / bound).max()))
        worst = max(worst, float((diff / bound).max()))
        if days == 0.0:
            assert (co["endnuc_coeff"] == 0).all() and (co["he4_coeff"] == 0).all() and (co["survivingfrac"] == 1).all()
    print(f"{g}: worst |sum of the nuclides - initial sum| / bound = {worst:.3f}")


def test_rows_are_in_path_order_with_the_he4_merge(setups, nets):
    net = nets["small"]
    model, dm, host = setups[("3d", "small")]
    r = host.rows()
    he4 = host.he4
    start, idx, typ = net["path_start"], net["path_nucindex"], net["path_last_decaytype"]
    ends = idx[start[1:] - 1]
    for nuc in range(len(net["nuc_z"])):
        got = list(zip(r["row_path"][r["row_start"][nuc]: r["row_start"][nuc + 1]], r["row_kind"][r["row_start"][nuc]: r["row_start"][nuc + 1]]))
        want = []
        for p in range(len(ends)):
            if ends[p] == nuc:
                want.append((p, 0))
            if nuc == he4 and typ[p] == abi.DECAYTYPE_ALPHA and ends[p] != he4:
                want.append((p, 1))
        assert [(int(a), int(b)) for a, b in got] == want, nuc
    nalpha = int((typ == abi.DECAYTYPE_ALPHA).sum())
    assert r["row_start"][he4 + 1] - r["row_start"][he4] == nalpha > 20
    Z = [int(z) for z in model["elem_anumber"]]
    assert list(r["nuc_element"]) == [Z.index(z) if z in Z else -1 for z in net["nuc_z"]]
    for el in range(len(Z)):
        assert list(r["elem_nuc"][r["elem_nuc_start"][el]: r["elem_nuc_start"][el + 1]]) == [i for i, z in enumerate(net["nuc_z"]) if z == Z[el]]
    # without He4 no row has an entry of kind 1
    assert (setups[("3d", "small_nohe4")][2].rows()["row_kind"] == 0).all()


def test_validate_refuses_malformed_networks(setups, nets):
    model, dm, host = setups[("1d", "small")]
    n, ne = int(model["npts_nonempty"]), int(model["nelements"])
    assert dc.validate(dm, n, ne) == ""

    def broken(**changes):
        d = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in dm.items()}
        for k, f in changes.items():
            d[k] = f(d[k])
        return dc.validate(d, n, ne)

    def short_path(start):  # path 3 loses all but its first nuclide's worth of entries
        s = start.copy()
        s[4:] -= s[4] - s[3] - 1
        return s

    assert broken(path_start=short_path).startswith("path 3: shorter than 2")

    def bad_index(idx):
        idx[dm["path_start"][5]] = len(dm["nuc_z"])
        return idx

    assert broken(path_nucindex=bad_index) == "path 5: a nuclide index out of range"
    p_long = int(np.argmax(np.diff(dm["path_start"])))
    mid = int(dm["path_nucindex"][dm["path_start"][p_long] + 3])

    def stable_mid(life):
        life[mid] = -1.0
        return life

    msg = broken(nuc_meanlife=stable_mid)
    assert msg.startswith("path ") and msg.endswith("a nuclide before the end with meanlife <= 0")
    other = int(dm["path_nucindex"][dm["path_start"][p_long] + 5])

    def equal_lives(life):
        life[mid] = life[other]
        return life

    msg = broken(nuc_meanlife=equal_lives)
    assert msg.startswith("path ") and "equal decay constants" in msg

    def neg_branch(b):
        b[7] = -0.5
        return b

    assert broken(path_branchproduct=neg_branch) == "path 7: a non-finite or negative branchproduct"

    def nan_life(life):
        life[0] = np.nan
        return life

    assert "non-finite mean life" in broken(nuc_meanlife=nan_life)

    def neg_x(x):
        x[2, 3] = -1e-3
        return x

    assert broken(initnucmassfrac=neg_x) == "initnucmassfrac: a non-finite or negative entry"
    assert "t_model" in broken(t_model=lambda t: float("inf"))
