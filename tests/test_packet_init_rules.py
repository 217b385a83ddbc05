"""The rules of artis_amd/csrc/packet_init.h (x86 build, tests/packet_init_host) against a numpy restatement written from the
reference's packet_init() (packet.cc:91-161, decay.cc:482, :1052-1080, :1347-1445, grid.cc:1577-1637, gammapkt.cc:869): np.cumsum for
every chain, abi.seed_packet_rng and a Python Xoshiro128++ step for the draws. No GPU."""
import math

import numpy as np
import pytest
from scipy import stats

import packet_init_common as pc
from artis_amd import abi

H = 6.6260755e-27
MH = 1.67352e-24
CLIGHT = 2.99792458e10
M32 = 0xFFFFFFFF
F32 = np.float32


# ---- the restatement
class Rng:
    """Xoshiro128++ (random.h:125) from a packet's seeded state; uniform() is rng_uniform (random.h:49): a float"""

    def __init__(self, state):
        self.s = [int(x) for x in state]

    def next(self) -> int:
        s = self.s
        x = (s[0] + s[3]) & M32
        result = ((((x << 7) | (x >> 25)) & M32) + s[0]) & M32
        t = (s[1] << 9) & M32
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = ((s[3] << 11) | (s[3] >> 21)) & M32
        return result

    def uniform(self) -> np.float32:
        return F32(self.next() >> 8) * F32(2.0 ** -24)

    def uniform_pos(self) -> np.float32:
        z = self.uniform()
        while not z > 0:
            z = self.uniform()
        return z


def decaychain_ref(lambdas, timediff):
    """decay.h:56 with the chain's end stable, and the clamps of decay_update.h"""
    lam = list(lambdas[:-1]) + [0.0]
    n = len(lam)
    lambdaproduct = 1.0
    for j in range(n - 1):
        lambdaproduct *= lam[j]
    s, maxabs = 0.0, 0.0
    for j in range(n):
        den = 1.0
        for p in range(n):
            if p != j:
                den *= lam[p] - lam[j]
        term = math.exp(-lam[j] * timediff) / den
        s += term
        maxabs = max(maxabs, abs(term))
    last = lambdaproduct * s
    if last < 0.0 or abs(s) <= n * 2.0 ** -52 * maxabs or lambdaproduct * maxabs < 2.2250738585072014e-308:
        return 0.0
    return last


def energy_vector_ref(dm, em, pm, tmin):
    """calc_energy_per_massoftopnuc_decaypath decay.cc:1067"""
    start, idx = np.asarray(dm["path_start"]), np.asarray(dm["path_nucindex"])
    life = np.asarray(dm["nuc_meanlife"], np.float64)
    t_model = float(dm["t_model"])
    t0 = t_model if pm["initial_packets_on"] else tmin
    E = np.zeros(len(start) - 1)
    for p in range(len(E)):
        nuc = idx[start[p]: start[p + 1]]
        lam = [1.0 / life[i] if life[i] > 0 else 0.0 for i in nuc]
        f = max(0.0, decaychain_ref(lam, pm["tmax"] - t_model) - decaychain_ref(lam, t0 - t_model))
        last = nuc[-2]
        endecay = float(em["nuc_endecay_gamma"][last]) + float(np.asarray(em["nuc_endecay_particle"]).reshape(-1, 6)[last, int(dm["path_last_decaytype"][p])])
        E[p] = float(dm["path_branchproduct"][p]) * f * (endecay / float(pm["nuc_decay_daughters_probsum"][last])) / (float(dm["nuc_a"][nuc[0]]) * MH)
    return E


def coords(model):
    nc = [int(x) for x in model["ncoordgrid"]]
    mins = [np.asarray(a, np.float64) for a in model["coord_pos_min_tmin"]]
    maxs = [np.concatenate([m[1:], [float(model["rmax"])]]) if len(m) else m for m in mins]
    return nc, mins, maxs


def cumulative_ref(model, dm, pm, E):
    """(endecay_per_mass, en_cumulative): decay.cc:1052 and packet.cc:116-131"""
    n = int(model["npts_nonempty"])
    top = np.asarray(dm["path_nucindex"])[np.asarray(dm["path_start"])[:-1]]
    X = np.asarray(dm["initnucmassfrac"], np.float32).reshape(n, -1)
    endecay = np.array([np.cumsum(np.concatenate([[0.0], X[c, top].astype(np.float64) * E]))[-1] for c in range(n)])
    nc, mins, maxs = coords(model)
    gt, ngrid = int(model["gridtype"]), int(model["ngrid"])
    cell = np.arange(ngrid)
    if gt == abi.GRID_CARTESIAN3D:
        dx = maxs[0][0] - mins[0][0]
        vol = np.full(ngrid, dx * dx * dx)
    elif gt == abi.GRID_CYLINDRICAL2D:
        ir = cell % nc[0]
        vol = (maxs[1][0] - mins[1][0]) * math.pi * (maxs[0][ir] * maxs[0][ir] - mins[0][ir] * mins[0][ir])
    else:
        vol = 4.0 / 3.0 * math.pi * (maxs[0] * maxs[0] * maxs[0] - mins[0] * mins[0] * mins[0])
    prop = np.asarray(model["propcell_nonemptymgi"])
    q = np.asarray(pm["initenergyq"], np.float64) if pm.get("initenergyq") is not None else np.zeros(n)
    rho = np.asarray(dm["rho_tmin"], np.float32).astype(np.float64)
    c = np.where(prop >= 0, prop, 0)
    terms = np.where(prop >= 0, vol * rho[c] * (endecay[c] + q[c]), 0.0)
    return endecay, np.cumsum(terms)


def packets_ref(model, dm, em, pm, E, en_cum, npackets, seed_base):
    """place_pellet packet.cc:54 and setup_radioactive_pellet decay.cc:1347 for the packets 0 .. npackets - 1 of a 3D grid"""
    assert int(model["gridtype"]) == abi.GRID_CARTESIAN3D
    pk = np.zeros(npackets, abi.PACKET_DTYPE)
    abi.seed_packet_rng(pk, seed_base)
    pk["pellet_nucindex"] = pk["pellet_decaytype"] = -1  # packet.h:152-153
    n = int(model["npts_nonempty"])
    tmin, tmax, t_model = float(model["tmin"]), float(pm["tmax"]), float(dm["t_model"])
    nc, mins, maxs = coords(model)
    prop = np.asarray(model["propcell_nonemptymgi"])
    start, idx = np.asarray(dm["path_start"]), np.asarray(dm["path_nucindex"])
    top = idx[start[:-1]]
    X = np.asarray(dm["initnucmassfrac"], np.float32).reshape(n, -1)
    life = np.asarray(dm["nuc_meanlife"], np.float64)
    engamma_all = np.asarray(em["nuc_endecay_gamma"], np.float64)
    enparticle_all = np.asarray(em["nuc_endecay_particle"], np.float64).reshape(-1, 6)
    gs, ge, gp = pm["gamma_start"], pm["gamma_energy"], pm["gamma_probability"]
    channel_on = pm.get("initenergyq") is not None
    etot = en_cum[-1]
    e_per = etot / npackets
    tdecaymin = tmin if not pm["initial_packets_on"] else t_model
    channel = np.zeros(npackets, np.int32)
    trials = np.zeros(npackets, np.int32)
    cums = {}
    for i in range(npackets):
        r = Rng(pk["rngstate"][i])
        cellindex = int(np.searchsorted(en_cum, r.uniform() * etot, side="right"))
        ix = [cellindex % nc[0], (cellindex // nc[0]) % nc[1], (cellindex // (nc[0] * nc[1])) % nc[2]]
        pos = [mins[a][ix[a]] + (r.uniform_pos() * (maxs[a][ix[a]] - mins[a][ix[a]])) for a in range(3)]
        c = int(prop[cellindex])
        if c not in cums:
            cum = np.cumsum(X[c, top].astype(np.float64) * E)
            cums[c] = np.append(cum, cum[-1] + pm["initenergyq"][c]) if channel_on else cum
        cum = cums[c]
        ch = int(np.searchsorted(cum, r.uniform() * cum[-1], side="right"))
        channel[i] = ch
        q = pk[i]
        q["cellindex"], q["number"], q["prop_time"], q["pos"] = cellindex, i, tmin, pos
        q["type"], q["e_cmf"] = abi.TYPE_RADIOACTIVE_PELLET, e_per
        if ch >= len(top):
            q["tdecay"], q["nu_cmf"] = tmin, e_per / H
        else:
            nuc = idx[start[ch]: start[ch + 1]]
            t = -1.0
            while t <= tdecaymin or t >= tmax:
                t = t_model
                for k in nuc[:-1]:
                    t -= life[k] * math.log(float(r.uniform_pos()))
                trials[i] += 1
            last, dt = int(nuc[-2]), int(dm["path_last_decaytype"][ch])
            engamma, enparticle = engamma_all[last], enparticle_all[last, dt]
            with np.errstate(invalid="ignore", divide="ignore"):
                particle = bool(r.uniform() >= np.float64(engamma) / np.float64(engamma + enparticle))
            if particle:
                nu = enparticle / H
            elif gs[last + 1] == gs[last]:
                nu = -1.0
            else:
                zrand = r.uniform()
                runtot = np.cumsum(gp[gs[last]: gs[last + 1]] * ge[gs[last]: gs[last + 1]] / engamma)
                hit = np.nonzero(zrand < runtot)[0]
                nu = ge[gs[last] + (hit[0] if len(hit) else len(runtot) - 1)] / H
            q["tdecay"], q["nu_cmf"], q["pellet_nucindex"], q["pellet_decaytype"], q["originated_from_particlenotgamma"] = t, nu, last, dt, particle
        pk["rngstate"][i] = r.s
    e_total = np.cumsum(pk["e_cmf"])[-1]
    e_ratio = etot / e_total
    pk["e_cmf"] *= e_ratio
    return pk, channel, trials, e_ratio


def host_population(gridtype, kind, initial, npackets, E=None, **kw):
    model, cs, ts, dm, em, pm = pc.case(gridtype, kind, initial)
    h = pc.HostPinit(dm, em, pm, model)
    E = h.energy() if E is None else E
    cells = h.cells(E)
    return (model, dm, em, pm), h, E, cells, h.run(npackets, **kw)


# ---- the vector, the cells, the packets
@pytest.mark.parametrize("kind,initial", [("small", True), ("small", False), ("medium", False)])
def test_energy_vector_is_the_restatements(kind, initial):
    model, cs, ts, dm, em, pm = pc.case(abi.GRID_CARTESIAN3D, kind, initial)
    E = pc.HostPinit(dm, em, pm, model).energy()
    ref = energy_vector_ref(dm, em, pm, float(model["tmin"]))
    assert np.array_equal(E.view(np.uint64), ref.view(np.uint64))
    assert np.all(np.isfinite(E)) and np.all(E >= 0) and np.count_nonzero(E) > len(E) // 2


@pytest.mark.parametrize("gridtype", [abi.GRID_SPHERICAL1D, abi.GRID_CYLINDRICAL2D, abi.GRID_CARTESIAN3D])
@pytest.mark.parametrize("kind,initial", [("small", True), ("medium", False)])
def test_cell_sums_and_en_cumulative_bit_for_bit(gridtype, kind, initial):
    model, cs, ts, dm, em, pm = pc.case(gridtype, kind, initial)
    h = pc.HostPinit(dm, em, pm, model)
    E = h.energy()
    got = h.cells(E)
    endecay, en_cum = cumulative_ref(model, dm, pm, E)
    assert np.array_equal(got["endecay_per_mass"].view(np.uint64), endecay.view(np.uint64))
    assert np.array_equal(got["en_cumulative"].view(np.uint64), en_cum.view(np.uint64))
    assert got["etot_simtime"] == en_cum[-1] > 0
    # empty cells and the cell without radioactive matter repeat the running value
    prop = np.asarray(model["propcell_nonemptymgi"])
    width = np.diff(np.concatenate([[0.0], en_cum]))
    assert np.all(width[prop < 0] == 0) and width[pc.propcell_of(model, pc.ZERO_CELL % int(model["npts_nonempty"]))] == 0


@pytest.mark.parametrize("kind,initial,npackets", [("small", True, 3000), ("small", False, 1500), ("medium", False, 1500)])
def test_packets_bit_for_bit_3d(kind, initial, npackets):
    (model, dm, em, pm), h, E, cells, got = host_population(abi.GRID_CARTESIAN3D, kind, initial, npackets)
    ref, channel, trials, e_ratio = packets_ref(model, dm, em, pm, E, cells["en_cumulative"], npackets, pc.SEED_BASE)
    pk = got["packets"]
    for f in ("cellindex", "number", "type", "pellet_nucindex", "pellet_decaytype", "originated_from_particlenotgamma", "rngstate"):
        assert np.array_equal(pk[f], ref[f]), f
    assert np.array_equal(got["channel"], channel) and np.array_equal(got["trials"], trials)
    for f in ("pos", "e_cmf", "nu_cmf", "tdecay", "prop_time"):
        assert np.array_equal(np.ascontiguousarray(pk[f]).view(np.uint64), np.ascontiguousarray(ref[f]).view(np.uint64)), f
    assert got["e_ratio"] == e_ratio and got["e_cmf_per_packet"] == cells["etot_simtime"] / npackets
    # what the restatement leaves to the rules: dir = pos / |pos|, e_rf = e_cmf / doppler, the defaults of packet.h
    r = np.sqrt(np.cumsum(pk["pos"] ** 2, axis=1)[:, -1])
    assert np.array_equal(pk["dir"], pk["pos"] / r[:, None])
    ndotv = np.cumsum(pk["dir"] * (pk["pos"] / float(model["tmin"])), axis=1)[:, -1]
    assert np.allclose(pk["e_rf"], pk["e_cmf"] / (1.0 - ndotv / CLIGHT), rtol=1e-14, atol=0)
    assert np.all(pk["emissiontype"] == abi.EMTYPE_NOTSET) and np.all(pk["trueemissiontype"] == abi.EMTYPE_NOTSET) and np.all(pk["next_trans"] == -1)
    assert np.all(np.isnan(pk["em_pos"])) and np.all(pk["em_time"] == -1) and np.all(pk["escape_time"] == -1) and np.all(pk["nu_rf"] == 0)
    if initial:
        assert np.count_nonzero(channel == h.np) > 10  # the initial-energy channel is drawn
        q = pk[channel == h.np]
        assert np.all(q["tdecay"] == model["tmin"]) and np.all(q["pellet_nucindex"] == -1) and np.all(q["pellet_decaytype"] == -1)
    assert np.count_nonzero(pk["nu_cmf"] == -1) > 0 and np.count_nonzero(pk["originated_from_particlenotgamma"]) > 0
    assert not np.any(pk["cellindex"] == pc.propcell_of(model, pc.ZERO_CELL))


@pytest.mark.parametrize("gridtype", [abi.GRID_SPHERICAL1D, abi.GRID_CYLINDRICAL2D])
def test_positions_lie_in_their_cells_1d_2d(gridtype):
    (model, dm, em, pm), h, E, cells, got = host_population(gridtype, "small", True, 4000)
    pk = got["packets"]
    nc, mins, maxs = coords(model)
    i0 = pk["cellindex"] % nc[0]
    r = np.sqrt(pk["pos"][:, 0] ** 2 + pk["pos"][:, 1] ** 2 + (pk["pos"][:, 2] ** 2 if gridtype == abi.GRID_SPHERICAL1D else 0.0))
    assert np.all(r >= mins[0][i0] * (1 - 1e-15)) and np.all(r <= maxs[0][i0] * (1 + 1e-15))
    if gridtype == abi.GRID_CYLINDRICAL2D:
        i1 = pk["cellindex"] // nc[0]
        assert np.all(pk["pos"][:, 2] >= mins[1][i1]) and np.all(pk["pos"][:, 2] <= maxs[1][i1])
    assert np.allclose(np.sum(pk["dir"] ** 2, axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.all(np.asarray(model["propcell_nonemptymgi"])[pk["cellindex"]] >= 0)


def test_result_does_not_depend_on_the_trial_budget():
    (model, dm, em, pm), h, E, cells, whole = host_population(abi.GRID_CARTESIAN3D, "small", True, 2000)
    cut = h.run(2000, budget=1)
    assert cut["calls"] > 1 and whole["calls"] == 1
    assert cut["packets"].tobytes() == whole["packets"].tobytes() and np.array_equal(cut["trials"], whole["trials"])
    assert h.run(2000, budget=1, max_calls=1)["calls"] == -1


# ---- lerp, the upper bound
def test_lerp_is_std_lerp():
    L = pc.lib()
    rng = np.random.default_rng(3)
    vals = [0.0, -0.0, 1.0, -1.0, 1e300, -1e300, 5e-324, 1e-300, 3.0, 2.5e15, 1.0 + 2.0 ** -52]
    ts = [0.0, 1.0, 0.5, 2.0 ** -24, 1 - 2.0 ** -24, 1.0 + 2.0 ** -52, 2.0, -1.0, 1e-300]
    cases = [(a, b, t) for a in vals for b in vals for t in ts]
    cases += [(a, a, t) for a in vals for t in ts]  # a == b
    cases += [tuple(x) for x in np.column_stack([rng.normal(0, 1e15, 4000), rng.normal(0, 1e15, 4000), rng.random(4000).astype(np.float32)])]
    cases += [(a ** 3, b ** 3, float(F32(t))) for a, b, t in rng.uniform(1e13, 4e14, (4000, 3)) / [1, 1, 4e14]]
    naive_differs = 0
    for a, b, t in cases:
        got, want = L.pinit_host_lerp(a, b, t), L.pinit_host_std_lerp(a, b, t)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64) or (math.isnan(got) and math.isnan(want)), (a, b, t)
        with np.errstate(all="ignore"):
            naive = np.float64(a) + np.float64(t) * (np.float64(b) - np.float64(a))
        naive_differs += not (naive == want or (np.isnan(naive) and math.isnan(want)))
    assert naive_differs > 0  # a + t (b - a) is not it
    assert L.pinit_host_lerp(3.0, 7.0, 0.0) == 3.0 and L.pinit_host_lerp(3.0, 7.0, 1.0) == 7.0 and L.pinit_host_lerp(-3.0, 7.0, 1.0) == 7.0


@pytest.mark.parametrize("kind,initial", [("small", False), ("small", True), ("medium", False), ("medium", True)])
def test_channel_upper_bound_on_ties_and_zero_widths(kind, initial):
    """X = 0.5 for half the nuclides and 0 for the rest, E a small integer or 0: the running sum is exact, many entries have zero width
    and the targets u * last of u = j / 4096 fall ON entries"""
    model, cs, ts, dm0, em, pm0 = pc.case(abi.GRID_CARTESIAN3D, kind, initial)
    dm, pm = dict(dm0), dict(pm0)
    n, nn = int(model["npts_nonempty"]), len(dm["nuc_z"])
    rng = np.random.default_rng(9)
    X = np.zeros((n, nn), np.float32)
    X[:, rng.random(nn) < 0.5] = 0.5
    dm["initnucmassfrac"] = X
    if initial:
        pm["initenergyq"] = np.full(n, 8.0)
    h = pc.HostPinit(dm, em, pm, model)
    E = rng.integers(0, 4, h.np).astype(np.float64) * 2.0
    E[: pc.stride() + 3] = 0.0  # the first block and a little more have no width at all
    top = np.asarray(dm["path_nucindex"])[np.asarray(dm["path_start"])[:-1]]
    total = float(np.sum(X[0, top].astype(np.float64) * E)) + (8.0 if initial else 0.0)
    last_wide = int(np.nonzero(X[0, top] > 0)[0][-1])
    E[last_wide] += 2.0 * (2.0 ** math.ceil(math.log2(total)) - total)  # the last entry is a power of two: j / 4096 of it is exact
    h.cells(E)
    cum = np.cumsum(X[0, top].astype(np.float64) * E)
    if initial:
        cum = np.append(cum, cum[-1] + 8.0)
    width = np.diff(np.concatenate([[0.0], cum]))
    ties = 0
    for j in range(4096):
        u = j / 4096.0
        target = u * cum[-1]
        want = int(np.searchsorted(cum, target, side="right"))
        ties += bool(np.any(cum == target))
        assert h.channel(0, u) == want == h.channel(0, u, full=True), j
        assert width[want] > 0  # a path with X[top] = 0 or E = 0 is never chosen
    assert ties >= 32
    assert h.channel(0, 0.0) == int(np.nonzero(width > 0)[0][0])  # draw 0.0: the first entry of positive width
    assert h.channel(0, 1 - 2.0 ** -24) == int(np.nonzero(width > 0)[0][-1])


# ---- refusals
def test_refusals():
    model, cs, ts, dm, em, pm = pc.case(abi.GRID_CARTESIAN3D, "small", True)
    life = np.asarray(dm["nuc_meanlife"])
    n, tmin, tm = int(model["npts_nonempty"]), float(model["tmin"]), float(dm["t_model"])
    rad = int(np.nonzero(life > 0)[0][2])
    with_lines = int(np.nonzero(np.diff(pm["gamma_start"]) > 0)[0][1])
    assert pc.validate(pm, life, n, tmin, tm) == ("", False)

    def bad(text, unsupported=False, t_min=tmin, t_model=tm, **change):
        q = dict(pm)
        for k, v in change.items():
            q[k] = v(np.array(q[k], copy=True)) if callable(v) else v
        got = pc.validate(q, life, n, t_min, t_model)
        assert text in got[0] and got[1] == unsupported, got

    def put(i, v):
        def f(a):
            a[i] = v
            return a
        return f

    bad("UNIFORM_PELLET_ENERGIES", unsupported=True, uniform_pellet_energies=0)
    bad(f"nuclide {rad}: it decays and its decay_daughters_probsum is not positive", nuc_decay_daughters_probsum=put(rad, 0.0))
    bad(f"nuclide {rad}: a negative or non-finite decay_daughters_probsum", nuc_decay_daughters_probsum=put(rad, -1.0))
    bad(f"nuclide {rad}: a negative or non-finite decay_daughters_probsum", nuc_decay_daughters_probsum=put(rad, np.nan))
    bad(f"nuclide {with_lines}: gamma_start is not monotone", gamma_start=put(with_lines + 1, int(pm["gamma_start"][with_lines]) - 1))
    bad(f"nuclide {with_lines}: a negative or non-finite line", gamma_energy=put(int(pm["gamma_start"][with_lines]), np.inf))
    bad(f"nuclide {with_lines}: a negative or non-finite line", gamma_probability=put(int(pm["gamma_start"][with_lines]), -0.1))
    bad("cell 3: a negative or non-finite initenergyq", initenergyq=put(3, -1.0))
    bad("needs initenergyq", initenergyq=None)
    bad("initenergyq without", initial_packets_on=0)
    bad("tmax <= tmin", tmax=tmin)
    bad("tmax <= tmin", tmax=np.inf)
    bad("t_model > tmin", t_model=tmin * 1.5)
    bad("max_trials_per_launch", max_trials_per_launch=-1)
    E = np.ones(5)
    E[3] = -1.0
    assert "path 3" in pc.lib().pinit_host_vector_validate(E.ctypes.data, 5).decode()
    assert pc.lib().pinit_host_vector_validate(np.ones(5).ctypes.data, 5).decode() == ""


# ---- one law that needs no restatement
def test_cells_and_decay_times_follow_their_distributions():
    """2e5 packets, seeds SEED_BASE .. SEED_BASE + 199999. The pellets per cell against diff(en_cumulative) / etot (cells that expect
    fewer than 20 in one bin): chi-square below its upper 1e-3 quantile. tdecay of the most frequent one-decay path against the exponential of the nuclide's mean life from t_model,
    truncated to (tdecaymin, tmax): KS distance below its upper 1e-3 quantile."""
    npackets = 200000
    (model, dm, em, pm), h, E, cells, got = host_population(abi.GRID_CARTESIAN3D, "small", False, npackets)
    pk = got["packets"]
    p = np.diff(np.concatenate([[0.0], cells["en_cumulative"]])) / cells["etot_simtime"]
    counts = np.bincount(pk["cellindex"], minlength=len(p))
    assert np.all(counts[p == 0] == 0)
    big = npackets * p > 20  # the cells that expect fewer (the thin outer ones) are pooled into one bin
    expected = np.append(npackets * p[big], npackets * np.sum(p[~big]))
    observed = np.append(counts[big], np.sum(counts[~big]))
    assert np.count_nonzero(big) > 50 and expected[-1] > 20 and np.sum(observed) == npackets
    chi2 = float(np.sum((observed - expected) ** 2 / expected))
    bound = stats.chi2.isf(1e-3, len(expected) - 1)
    print(f"chi-square {chi2:.1f} of {len(expected) - 1} degrees of freedom, bound {bound:.1f}")
    assert chi2 < bound
    length = np.diff(np.asarray(dm["path_start"]))
    ch = got["channel"]
    one = np.bincount(ch[length[ch] == 2], minlength=h.np)
    path = int(np.argmax(one))
    tau = float(dm["nuc_meanlife"][dm["path_nucindex"][dm["path_start"][path]]])
    t = np.sort(pk["tdecay"][ch == path])
    t0, t1, tm = float(model["tmin"]), float(pm["tmax"]), float(dm["t_model"])
    assert len(t) > 5000 and t[0] > t0 and t[-1] < t1
    cdf = (np.exp(-(t0 - tm) / tau) - np.exp(-(t - tm) / tau)) / (np.exp(-(t0 - tm) / tau) - np.exp(-(t1 - tm) / tau))
    i = np.arange(1, len(t) + 1)
    ks = float(max(np.max(i / len(t) - cdf), np.max(cdf - (i - 1) / len(t))))
    ks_bound = float(stats.kstwo.isf(1e-3, len(t)))
    print(f"KS distance {ks:.5f} of {len(t)} packets of path {path}, bound {ks_bound:.5f}")
    assert ks < ks_bound
    # the energies: every packet carries etot / npackets after the normalisation, up to the rounding of its two factors
    assert np.all(np.abs(pk["e_cmf"] / got["e_cmf_per_packet"] - 1) < 1e-10) and abs(np.sum(pk["e_cmf"]) / cells["etot_simtime"] - 1) < 1e-10
