"""The rules of the deposition rates and thickness flags (artis_amd/csrc/deposition.h) in their x86 build (tests/deposition_host): the
power vectors, the per-cell bodies and the timestep totals against a sequential float64 restatement of decay.cc:1105-1183,
nonthermal.cc:2340-2380, sn3d.cc:240-286 and :532-563 and update_grid.cc:606-627 written here; the walk over the radioactive nuclides
against the walk over all of them; known answers; the law that ties the cells' analytic rates to the totals; the scheme switch, the
thickness flags, the validator and the row builder under the sanitizers. No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import decay_common as dc
import deposition_common as dp
from artis_amd import abi, synth

DAY, EPS = dp.DAY, dp.EPS
GRIDS = {"3d": abi.GRID_CARTESIAN3D, "2d": abi.GRID_CYLINDRICAL2D, "1d": abi.GRID_SPHERICAL1D}
ZERO_CELL = 2  # the cell whose X is all zero
PARTICLE_TYPE = (abi.DECAYTYPE_BETAPLUS, abi.DECAYTYPE_BETAMINUS, abi.DECAYTYPE_ALPHA, abi.DECAYTYPE_SPONTFISSION)


def grid(g, options="classic"):
    if g == "2d":
        return synth.build("small", ncoord=5, gridtype=abi.GRID_CYLINDRICAL2D, options=options)
    return dc.grid(GRIDS[g], options)


@pytest.fixture(scope="module")
def nets():
    return {k: synth.decay_network(k) for k in dp.NETWORKS}


class Setup:
    def __init__(self, g, net, preset="classic"):
        self.model, self.cs, self.ts, aux = grid(g)
        self.dm = synth.decay_model(self.model, self.cs, aux, net, t_model=dp.T_MODEL)
        self.dm["initnucmassfrac"][ZERO_CELL, :] = 0.0
        self.em = synth.deposition_model(self.model, net)
        self.n = int(self.model["npts_nonempty"])
        self.decay = dc.HostDecay(self.dm, self.model)
        self.host = dp.HostDep(self.dm, self.em, self.model, preset)
        rng = np.random.default_rng(3)
        self.kappagrey = rng.uniform(0.05, 0.3, self.n).astype(np.float32)
        self.raw = dp.raw_estimators(self.n)

    def at(self, days):
        """(t_mid, coefficients, rho) of the decay update the deposition update works on"""
        t_mid = dp.T_MODEL + days * DAY
        co = self.decay.coeffs(t_mid)
        return t_mid, co, self.decay.cells(t_mid, co, nuclides=False)["rho"]

    def step(self, t_mid, nts_next=3, num_grey=5, thick=1e30, thick_vpkt=0.0, nprocs=2):
        return dp.step_params(self.model, t_mid, 0.9 * t_mid, 0.1 * t_mid, nts_next, num_grey, thick, thick_vpkt, nprocs)


@pytest.fixture(scope="module")
def setups(nets):
    cache = {}

    def get(g, netkind, preset="classic"):
        if (g, netkind, preset) not in cache:
            cache[(g, netkind, preset)] = Setup(g, nets[netkind], preset)
        return cache[(g, netkind, preset)]

    return get


def restate_vectors(dm, em, co):
    """decay.cc:1105-1168 with sequential float64 operations (vectors over the eleven energies)"""
    life = np.asarray(dm["nuc_meanlife"], np.float64)
    mass = np.asarray(dm["nuc_a"], np.float64) * synth.MH
    part, q, br = (np.asarray(em[k], np.float64).reshape(-1, 6) for k in ("nuc_endecay_particle", "nuc_endecay_q", "nuc_branchprob"))
    energy = np.stack([np.asarray(em["nuc_endecay_gamma"], np.float64)] + [part[:, t] * br[:, t] for t in PARTICLE_TYPE] + [q[:, t] * br[:, t] for t in range(6)])
    safe = np.where(life > 0, life, 1.0)
    pcm = np.where(life > 0, energy / safe / mass, 0.0)
    P = pcm * np.asarray(co["survivingfrac"])[None, :]
    start, idx = dm["path_start"], dm["path_nucindex"]
    for p in range(len(start) - 1):
        top, end = idx[start[p]], idx[start[p + 1] - 1]
        P[:, top] = P[:, top] + pcm[:, end] * co["endnuc_coeff"][p]
    return P


def restate_cells(s, step, P, rho, instant):
    """decay.cc:1173, sn3d.cc:544-558, nonthermal.cc:2340-2380 and update_grid.cc:606-627, sequential float64 (vectors over the cells)"""
    t_mid, tmin, rmax, prev_mid, prev_width, nprocs, nts_next, num_grey, thick, thick_vpkt = step
    X = np.asarray(s.dm["initnucmassfrac"], np.float32).astype(np.float64)
    sums = np.zeros((5, s.n))
    for nuc in range(X.shape[1]):
        for ch in range(5):
            sums[ch] = sums[ch] + P[ch, nuc] * X[:, nuc]
    rho32 = np.asarray(rho, np.float32)
    eps = rho32.astype(np.float64)[None, :] * sums
    r = prev_mid / tmin
    dV = np.asarray(s.em["assocvolume_tmin"]) * (r * r * r)
    norm = 1 / dV / prev_width / int(nprocs)
    dep = np.zeros((5, s.n))
    dep[0] = s.raw[0] * norm
    for ch in (1, 2, 3):
        dep[ch] = eps[ch] if instant else s.raw[ch] * norm
    dep[4] = eps[4]
    tratmid = t_mid / tmin
    d = (rmax * tratmid) - np.asarray(s.em["radial_pos_tmin"]) * tratmid
    dist = np.where(d > 0, d, 0.0)
    grey = ((s.kappagrey * rho32).astype(np.float64) * dist).astype(np.float32)
    flags = np.where((grey.astype(np.float64) >= thick) & (nts_next < num_grey), abi.CELL_THICK, abi.CELL_THIN).astype(np.int32)
    return dict(eps_ana=eps, dep=dep, ntlepton_deposition_rate_density=(dep[0] + dep[1]) + dep[2], grey_depth=grey, thick=flags)


def restate_totmass(s):
    X = np.asarray(s.dm["initnucmassfrac"], np.float32).astype(np.float64)
    cellmass = np.asarray(s.dm["rho_tmin"], np.float32).astype(np.float64) * np.asarray(s.em["assocvolume_tmin"])
    tot, mtot = np.zeros(X.shape[1]), 0.0
    for c in range(s.n):
        mtot += float(cellmass[c])
        tot = tot + cellmass[c] * X[c]
    return tot, mtot


def restate_totals(s, nprocs, P, tot):
    out = []
    for k in range(4):
        acc = 0.0
        for c in range(s.n):
            acc += float(s.raw[k, c]) / nprocs
        out.append(acc)
    for v in range(abi.DEP_NVECTORS):
        acc = 0.0
        for nuc in range(len(tot)):
            acc += float(P[v, nuc]) * float(tot[nuc])
        out.append(acc)
    return np.array(out)


CASES = [("3d", "small", 20.0), ("3d", "medium", 0.0), ("2d", "small_nohe4", 300.0), ("2d", "medium", 20.0), ("1d", "small", 0.0),
         ("1d", "small_nohe4", 20.0), ("1d", "medium", 300.0)]


def test_networks_and_grids_are_the_ones_the_tests_need(nets, setups):
    assert len(nets["medium"]["nuc_z"]) == 300 and len(nets["medium"]["path_start"]) - 1 == 2100
    s = setups("3d", "medium")
    D = dp.depth()
    assert s.host.nrad == 280 and s.host.nrad > 4 * D and s.host.nrad % D != 0
    assert 0 < setups("3d", "small_nohe4").host.nrad < D  # ... and a walk shorter than one block
    assert s.n % 64 != 0 and setups("1d", "small").n == 5
    assert (s.dm["initnucmassfrac"][ZERO_CELL] == 0).all() and (s.dm["initnucmassfrac"][ZERO_CELL + 1] > 0).any()
    em = synth.decay_energies(nets["small"])
    br = em["nuc_branchprob"]
    life = nets["small"]["nuc_meanlife"]
    assert (br[life <= 0] == 0).all() and np.allclose(br[life > 0].sum(axis=1), 1.0)
    assert (br[:, abi.DECAYTYPE_ELECTRONCAPTURE] > 0).any() and (em["nuc_endecay_particle"][:, abi.DECAYTYPE_ELECTRONCAPTURE] == 0).all()
    assert (em["nuc_endecay_particle"][life <= 0] == 0).all() and (em["nuc_endecay_gamma"][life <= 0] == 0).all()
    for g in GRIDS:
        model = grid(g)[0]
        rp = synth.radial_pos_tmin(model)
        assert rp.shape == (int(model["npts_nonempty"]),) and (rp > 0).all() and (rp < float(model["rmax"])).all()


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]:g}d" for c in CASES])
def test_vectors_cells_and_totals_bit_identical_to_a_sequential_restatement(setups, case):
    g, netkind, days = case
    s = setups(g, netkind)
    t_mid, co, rho = s.at(days)
    P = s.host.vectors(co)
    want_P = restate_vectors(s.dm, s.em, co)
    assert P.tobytes() == want_P.tobytes(), int((P != want_P).sum())
    assert s.host.vectors_validate(P) == ""
    stable = np.asarray(s.dm["nuc_meanlife"]) <= 0
    assert stable.any() and (P[:, stable] == 0).all() and not np.signbit(P[:, stable]).any() and (P[0, ~stable] > 0).any()
    step = s.step(t_mid)
    got = s.host.cells(step, P, rho, s.kappagrey, s.raw)
    want = restate_cells(s, step, P, rho, instant=True)
    for k, v in want.items():
        assert got[k].tobytes() == v.tobytes(), (k, int((got[k] != v).sum()))
    assert (got["eps_ana"][:, ZERO_CELL] == 0).all() and (got["eps_ana"][0, ZERO_CELL + 1] > 0)
    # walking only the radioactive nuclides is walking every nuclide
    assert s.host.nrad < s.host.nn
    every = s.host.cells(step, P, rho, s.kappagrey, s.raw, all_nuclides=True)
    for k, v in every.items():
        assert got[k].tobytes() == v.tobytes(), (k, "all nuclides")
    tot, mtot = s.host.totmass()
    want_tot, want_mtot = restate_totmass(s)
    assert tot.tobytes() == want_tot.tobytes() and mtot == want_mtot
    totals = s.host.totals(2, P, s.raw, tot)
    assert totals.tobytes() == restate_totals(s, 2, P, tot).tobytes()
    if days == 0.0:  # t_mid == t_model: nothing has decayed, the vectors are the nuclides' own powers
        assert (co["endnuc_coeff"] == 0).all() and (co["survivingfrac"] == 1).all()


def test_the_identity_is_about_order(setups):
    """the same cell sums taken in reversed nuclide order differ somewhere"""
    s = setups("3d", "medium")
    t_mid, co, rho = s.at(20.0)
    P = s.host.vectors(co)
    got = s.host.cells(s.step(t_mid), P, rho, s.kappagrey, s.raw)["eps_ana"]
    X = np.asarray(s.dm["initnucmassfrac"], np.float32).astype(np.float64)
    rev = np.zeros(s.n)
    for nuc in reversed(range(X.shape[1])):
        rev = rev + P[0, nuc] * X[:, nuc]
    assert (rho.astype(np.float64) * rev != got[0]).any()


def _tiny(nucs, paths):
    """a hand-made network: nucs [(z, a, meanlife)], paths [(nuclide indices, branchproduct, last decay type)]"""
    start = np.concatenate([[0], np.cumsum([len(p[0]) for p in paths])]).astype(np.int32)
    return dict(nuc_z=np.array([n[0] for n in nucs], np.int32), nuc_a=np.array([n[1] for n in nucs], np.int32),
                nuc_meanlife=np.array([n[2] for n in nucs], np.float64), path_start=start,
                path_nucindex=np.array([i for p in paths for i in p[0]], np.int32), path_branchproduct=np.array([p[1] for p in paths], np.float64),
                path_last_decaytype=np.array([p[2] for p in paths], np.int32))


def _tiny_setup(net, egamma):
    model, cs, ts, aux = grid("1d")
    dm = synth.decay_model(model, cs, aux, net, t_model=dp.T_MODEL)
    em = synth.deposition_model(model, net)
    em["nuc_endecay_gamma"] = np.asarray(egamma, np.float64)
    return model, dm, em, dc.HostDecay(dm, model), dp.HostDep(dm, em, model)


def test_known_answer_single_nuclide():
    """eps_gamma = e / tau / m x exp(-t / tau) x X x rho. The surviving fraction is a one-term Bateman sum: the bar of
    tests/test_decay_update_rules.py, 4 (L + x_dom) 2^-52 scale with L = 1, x_dom = t / tau and scale = exp(-t / tau), i.e. a relative
    4 (1 + t / tau) 2^-52; the two divisions and three products of the exact factors (and the float-to-double casts, which are exact)
    round once each, at most 2^-53 relative each, on either side: 2^-52 each covers both sides."""
    tau, e = 8.80 * DAY, 2.7e-6
    net = _tiny([(28, 56, tau), (27, 56, -1.0)], [([0, 1], 1.0, abi.DECAYTYPE_ELECTRONCAPTURE)])
    model, dm, em, decay, host = _tiny_setup(net, [e, 0.0])
    n = int(model["npts_nonempty"])
    for days in (0.0, 2.0, 30.0, 300.0):
        t_mid = dp.T_MODEL + days * DAY
        co = decay.coeffs(t_mid)
        rho = decay.cells(t_mid, co, nuclides=False)["rho"]
        P = host.vectors(co)
        out = host.cells(dp.step_params(model, t_mid, 0.9 * t_mid, 0.1 * t_mid, 1, 0, 1.0), P, rho, np.full(n, 0.1, np.float32), np.zeros((4, n)))
        t = days * DAY
        X = np.asarray(dm["initnucmassfrac"], np.float32).astype(np.float64)[:, 0]
        want = e / tau / (56 * synth.MH) * math.exp(-t / tau) * X * rho.astype(np.float64)
        tol = (4 * (1 + t / tau) + 5) * EPS * want
        assert (want > 0).all() and (np.abs(out["eps_ana"][0] - want) <= tol).all(), days
        assert (out["eps_ana"][1:] == 0).all()


def test_known_answer_two_step_chain():
    """A -> B -> C (stable), X in A only: eps_gamma = rho X_A [e_A / tau_A / m_A exp(-t / tau_A) + e_B / tau_B / m_B x (m_B / m_A) x
    lambda_A / (lambda_B - lambda_A) (exp(-lambda_A t) - exp(-lambda_B t))]. The first term as in the single-nuclide test. The second
    is the path's coefficient times exact factors: the coefficient is within the bar of tests/test_decay_update_rules.py, 4 (L +
    x_dom) 2^-52 scale x A_B / A_A, of the exact Bateman sum, and so is the closed form evaluated here in float64 (the same terms):
    twice the bar between them, carried through e_B / tau_B / m_B x X x rho; five more roundings for the products, divisions and the
    addition of the two terms."""
    ta, tb, ea, eb = 8.80 * DAY, 113.7 * DAY, 2.7e-6, 5.9e-6
    net = _tiny([(28, 56, ta), (27, 56, tb), (26, 56, -1.0)],
                [([0, 1], 1.0, abi.DECAYTYPE_ELECTRONCAPTURE), ([0, 1, 2], 1.0, abi.DECAYTYPE_ELECTRONCAPTURE), ([1, 2], 1.0, abi.DECAYTYPE_ELECTRONCAPTURE)])
    model, dm, em, decay, host = _tiny_setup(net, [ea, eb, 0.0])
    dm["initnucmassfrac"][:, 1:] = 0.0
    decay, host = dc.HostDecay(dm, model), dp.HostDep(dm, em, model)
    n = int(model["npts_nonempty"])
    m = 56 * synth.MH
    la, lb = 1.0 / ta, 1.0 / tb
    for days in (2.0, 30.0, 300.0):
        t_mid = dp.T_MODEL + days * DAY
        co = decay.coeffs(t_mid)
        rho = decay.cells(t_mid, co, nuclides=False)["rho"]
        out = host.cells(dp.step_params(model, t_mid, 0.9 * t_mid, 0.1 * t_mid, 1, 0, 1.0), host.vectors(co), rho, np.full(n, 0.1, np.float32), np.zeros((4, n)))
        t = days * DAY
        X = np.asarray(dm["initnucmassfrac"], np.float32).astype(np.float64)[:, 0]
        xr = X * rho.astype(np.float64)
        first = ea / ta / m * math.exp(-la * t) * xr
        second = eb / tb / m * (la / (lb - la) * (math.exp(-la * t) - math.exp(-lb * t))) * xr
        bar_coeff = 4 * (2 + co["path_x_dom"][0]) * EPS * co["path_scale"][0]
        tol = (4 * (1 + t / ta) + 5) * EPS * first + 2 * bar_coeff * (eb / tb / m) * xr + 5 * EPS * (first + second)
        assert (second > 0).all() and (np.abs(out["eps_ana"][0] - (first + second)) <= tol).all(), days


@pytest.mark.parametrize("g,netkind", [("3d", "medium"), ("2d", "small"), ("1d", "small_nohe4")])
def test_cells_and_totals_agree_up_to_summation_order(setups, g, netkind):
    """Per channel sum_cells eps_ana / rho x rho_tmin x assocvolume_tmin is the totmassnuclide product: both are the sum of P[nuc] x
    X[cell][nuc] x cellmass over cells and nuclides, taken in another order. Every partial sum of non-negative terms is off by at most
    its number of additions x 2^-52 x the sum: (ncell + nnuclides) x 2^-52 x the sum of the terms."""
    s = setups(g, netkind)
    t_mid, co, rho = s.at(20.0)
    P = s.host.vectors(co)
    out = s.host.cells(s.step(t_mid), P, rho, s.kappagrey, s.raw)
    tot, mtot = s.host.totmass()
    totals = s.host.totals(1, P, s.raw, tot)
    X = np.asarray(s.dm["initnucmassfrac"], np.float32).astype(np.float64)
    cellmass = np.asarray(s.dm["rho_tmin"], np.float32).astype(np.float64) * np.asarray(s.em["assocvolume_tmin"])
    for ch in range(5):
        lhs = float(np.sum(out["eps_ana"][ch] / rho.astype(np.float64) * cellmass))
        terms = float(np.sum(cellmass[:, None] * X * P[ch][None, :]))
        assert abs(lhs - totals[4 + ch]) <= (s.n + s.host.nn) * EPS * terms, ch
        assert terms > 0 or ch != 0  # (the medium network has beta- decays only: its positron, alpha and fission channels are empty)
    assert abs(mtot - cellmass.sum()) <= s.n * EPS * mtot


def test_scheme_switch(setups):
    """INSTANTFULLDEPOSITION (classic) takes the analytic rates for positron, electron and alpha; the time-dependent build
    (kilonova_lte) the estimators"""
    assert dp.lib("classic").dep_host_instantfulldeposition() == 1 and dp.lib("kilonova_lte").dep_host_instantfulldeposition() == 0
    a, b = setups("3d", "small", "classic"), setups("3d", "small", "kilonova_lte")
    t_mid, co, rho = a.at(20.0)
    P = a.host.vectors(co)
    step = a.step(t_mid)
    oa, ob = a.host.cells(step, P, rho, a.kappagrey, a.raw), b.host.cells(step, P, rho, b.kappagrey, b.raw)
    want_b = restate_cells(b, step, P, rho, instant=False)
    for k, v in want_b.items():
        assert ob[k].tobytes() == v.tobytes(), k
    assert oa["eps_ana"].tobytes() == ob["eps_ana"].tobytes() and oa["dep"][0].tobytes() == ob["dep"][0].tobytes()
    for ch in (1, 2, 3):
        assert oa["dep"][ch].tobytes() == oa["eps_ana"][ch].tobytes() and (ob["dep"][ch] != oa["dep"][ch]).any()
    assert oa["dep"][4].tobytes() == oa["eps_ana"][4].tobytes() == ob["dep"][4].tobytes()
    assert (oa["ntlepton_deposition_rate_density"] != ob["ntlepton_deposition_rate_density"]).any()


@pytest.mark.parametrize("g", list(GRIDS))
def test_thickness(setups, nets, g):
    s = setups(g, "small")
    t_mid, co, rho = s.at(20.0)
    P = s.host.vectors(co)
    depth = s.host.cells(s.step(t_mid), P, rho, s.kappagrey, s.raw)["grey_depth"]
    tau = float(np.median(depth))
    assert depth.min() < tau < depth.max()
    grey = s.host.cells(s.step(t_mid, nts_next=4, num_grey=5, thick=tau), P, rho, s.kappagrey, s.raw)
    assert grey["grey_depth"].tobytes() == depth.tobytes()
    assert (grey["thick"] == abi.CELL_THICK).any() and (grey["thick"] == abi.CELL_THIN).any()
    assert np.array_equal(grey["thick"] == abi.CELL_THICK, depth.astype(np.float64) >= tau)
    late = s.host.cells(s.step(t_mid, nts_next=5, num_grey=5, thick=tau), P, rho, s.kappagrey, s.raw)
    assert (late["thick"] == abi.CELL_THIN).all()
    # a build with virtual packets: cells above their own limit that are not THICK are THICK_VPKT_ONLY
    low = float(0.5 * (np.sort(depth.astype(np.float64))[0] + np.sort(depth.astype(np.float64))[1]))  # between the two thinnest cells
    assert dp.lib("ci_classic_vpkt").dep_host_vpkt_on() == 1 and dp.lib("classic").dep_host_vpkt_on() == 0
    v = dp.HostDep(s.dm, s.em, s.model, "ci_classic_vpkt")
    vp = v.cells(s.step(t_mid, nts_next=4, num_grey=5, thick=tau, thick_vpkt=low), P, rho, s.kappagrey, s.raw)
    d64 = depth.astype(np.float64)
    want = np.where(d64 >= tau, abi.CELL_THICK, np.where(d64 > low, abi.CELL_THICK_VPKT_ONLY, abi.CELL_THIN))
    assert np.array_equal(vp["thick"], want) and all((want == k).any() for k in (abi.CELL_THIN, abi.CELL_THICK, abi.CELL_THICK_VPKT_ONLY))
    # a corner cell beyond rmax has depth 0 (the reference clamps the distance to the observer)
    em = dict(s.em)
    em["radial_pos_tmin"] = np.array(em["radial_pos_tmin"], copy=True)
    em["radial_pos_tmin"][0] = 1.2 * float(s.model["rmax"])
    corner = dp.HostDep(s.dm, em, s.model).cells(s.step(t_mid, thick=tau), P, rho, s.kappagrey, s.raw)
    assert corner["grey_depth"][0] == 0 and not np.signbit(corner["grey_depth"][0]) and corner["thick"][0] == abi.CELL_THIN
    assert corner["grey_depth"][1:].tobytes() == depth[1:].tobytes()


def test_validate_refuses_malformed_models(setups):
    s = setups("1d", "small")
    nn = s.host.nn
    assert dp.validate(s.em, nn, s.n) == ""

    def broken(key, index, value, nnuclides=nn, ncell=s.n):
        em = {k: np.array(v, copy=True) for k, v in s.em.items()}
        if key:
            em[key].reshape(-1)[index] = value
        return dp.validate(em, nnuclides, ncell)

    assert broken("nuc_endecay_gamma", 3, -1e-7) == "nuclide 3: a negative or non-finite endecay_gamma"
    assert broken("nuc_endecay_particle", 6 * 4 + 2, np.inf) == "nuclide 4: a negative or non-finite endecay_particle"
    assert broken("nuc_endecay_q", 6 * 5 + 1, np.nan) == "nuclide 5: a negative or non-finite endecay_q"
    assert broken("nuc_branchprob", 6 * 7 + 3, 1.5) == "nuclide 7: a branch probability outside [0, 1]"
    assert broken("nuc_branchprob", 6 * 7 + 3, -0.1) == "nuclide 7: a branch probability outside [0, 1]"
    assert broken("nuc_branchprob", 6 * 7 + 3, np.nan) == "nuclide 7: a branch probability outside [0, 1]"
    assert "assocvolume_tmin" in broken("assocvolume_tmin", 1, 0.0) and "cell 1" in broken("assocvolume_tmin", 1, -2.0)
    assert "radial_pos_tmin" in broken("radial_pos_tmin", 2, -1.0) and "radial_pos_tmin" in broken("radial_pos_tmin", 2, np.inf)
    assert "nnuclides" in broken(None, 0, 0, nnuclides=nn + 1) and "npts_nonempty" in broken(None, 0, 0, ncell=s.n + 1)
    em = dict(s.em)
    em["nuc_endecay_q"] = None
    assert "required" in dp.validate(em, nn, s.n)
    # handed-in vectors: as they are, so they must be usable as they are
    t_mid, co, rho = s.at(20.0)
    P = s.host.vectors(co)
    stable = int(np.nonzero(np.asarray(s.dm["nuc_meanlife"]) <= 0)[0][0])
    for (v, nuc, value, text) in ((0, 1, -1.0, "nuclide 1: a negative"), (10, 2, np.nan, "nuclide 2: a negative"), (3, stable, 1.0, "stable")):
        Q = P.copy()
        Q[v, nuc] = value
        assert text in s.host.vectors_validate(Q)


def test_rows_are_in_path_order(setups, nets):
    net = nets["small"]
    r = setups("3d", "small").host.rows()
    start, idx = net["path_start"], net["path_nucindex"]
    tops, ends = idx[start[:-1]], idx[start[1:] - 1]
    for nuc in range(len(net["nuc_z"])):
        k0, k1 = r["top_start"][nuc], r["top_start"][nuc + 1]
        want = [p for p in range(len(tops)) if tops[p] == nuc]
        assert list(r["top_path"][k0:k1]) == want and list(r["top_end"][k0:k1]) == [int(ends[p]) for p in want]
    assert list(r["rad_nuc"]) == [i for i, life in enumerate(net["nuc_meanlife"]) if life > 0]
    assert np.diff(r["top_start"]).max() > 10


def test_row_builder_under_the_sanitizers(tmp_path):
    """tests/deposition_host/rows_main.cc, a program of its own built with -fsanitize=address,undefined, on the three networks"""
    subprocess.check_call(["make", "-C", dp.HOSTDIR, "rows_sanitized"], stdout=subprocess.DEVNULL)
    for kind in dp.NETWORKS:
        dc.dump_network(synth.decay_network(kind), [14, 26, 27], str(tmp_path / f"{kind}.txt"))
    out = subprocess.run([os.path.join(dp.HOSTDIR, "rows_sanitized")] + [str(tmp_path / f"{k}.txt") for k in dp.NETWORKS], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("6 of 6 malformed copies refused") == 3 and "280 radioactive" in out.stdout
