"""The pellet initialisation on the device (artis_amd_packet_init*) against the x86 build of the same rules (tests/packet_init_host):
with the host's energy vector handed in every discrete field, the generator state, the energies, en_cumulative and the 3D positions
bit for bit, what goes through log / cbrt / sin / cos within a measured rounding bound; the device's own vector to the Bateman sum's
bound; the continuation launches, the installation as the resident population, and the refusals.

The rounding bounds. This ROCm ships no table of its math functions' ulp errors, so the worst difference between the device and the
x86 build was measured on the populations of this file (all grids, both networks, both channel settings, 20 000 packets each), in
units of 2^-53 times the quantity's natural scale, and four times the measured figure is allowed (a rounding difference has no tail
beyond a few ulps; a wrong formula is off by orders of magnitude):
  tdecay   |d| / sum over the accepted trial's terms of (meanlife |log u|
           + 2 |t after the subtraction|): log's last bits, and the last bit
           of every subtraction, which can round the other way                 measured 1.24   allowed 4.96
  pos      |d pos_i| / |pos| (1D and 2D; 0 in 3D)                              measured 5.36   allowed 21.44
  dir      |d dir_i| (1D and 2D; 0 in 3D)                                      measured 3.00   allowed 12
  e_rf     |d| / e_rf (1D and 2D; 0 in 3D)                                     measured 2.00   allowed 8
A packet is undecided when one of its x86 trial times lies within ULP_TDECAY 2^-53 times that trial's unit of tdecaymin
or tmax: a last-bit difference could flip the acceptance and with it every later draw. Such packets are left out, at most 2 per
test, and the x86 populations used here have none (test_host_populations_have_no_undecided_packet, on the CPU)."""
import functools

import numpy as np
import pytest

import decay_common as dc
import packet_init_common as pc
from artis_amd import abi, synth

U = 2.0 ** -53
# measured worst device - x86 differences in units of 2^-53 (see above), and the allowed four times of them
MEASURED_TDECAY, MEASURED_POS, MEASURED_DIR, MEASURED_ERF = 1.24, 5.36, 3.0, 2.0
ULP_TDECAY, ULP_POS, ULP_DIR, ULP_ERF = 4 * MEASURED_TDECAY, 4 * MEASURED_POS, 4 * MEASURED_DIR, 4 * MEASURED_ERF
NPK = 20000
GRIDS = {"1d": abi.GRID_SPHERICAL1D, "2d": abi.GRID_CYLINDRICAL2D, "3d": abi.GRID_CARTESIAN3D}
# (grid, network, initial-energy channel)
CASES = [("3d", "small", True), ("3d", "medium", False), ("1d", "small", False), ("1d", "medium", True), ("2d", "small", True), ("2d", "medium", False)]
DISCRETE = ("cellindex", "number", "type", "pellet_nucindex", "pellet_decaytype", "originated_from_particlenotgamma", "rngstate", "next_trans", "nscatterings",
            "emissiontype", "trueemissiontype", "absorptiontype", "escape_type")
EXACT = ("prop_time", "nu_cmf", "e_cmf", "nu_rf", "em_time", "trueem_time", "escape_time", "absorptionfreq", "stokes_q", "stokes_u")


@functools.lru_cache(maxsize=None)
def host_reference(grid: str, kind: str, initial: bool, npackets: int = NPK):
    """the x86 population of a case, made once: (E, cells, run with margins)"""
    model, cs, ts, dm, em, pm = pc.case(GRIDS[grid], kind, initial)
    h = pc.HostPinit(dm, em, pm, model)
    E = h.energy()
    return E, h.cells(E), h.run(npackets, margins=True)


def undecided(ref) -> np.ndarray:
    return ref["margin"] < ULP_TDECAY * U


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_host_populations_have_no_undecided_packet(case):
    """(CPU) at SEED_BASE no x86 trial time lies within the bound of tdecaymin or tmax: the GPU comparisons below leave nothing out"""
    E, cells, ref = host_reference(*case)
    assert not undecided(ref).any(), np.nonzero(undecided(ref))[0]
    assert np.all(ref["tdecay_unit"][ref["channel"] < len(E)] > 0)


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


def make_engine(engine_mod, grid, kind, initial, **pm_change):
    model, cs, ts, dm, em, pm = pc.case(GRIDS[grid], kind, initial)
    eng = engine_mod.Engine(model)
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    eng.packet_init_setup({**pm, **pm_change})
    return eng


def download(eng, npackets):
    pk = np.zeros(npackets, abi.PACKET_DTYPE)
    eng.download_packets(pk)
    return pk, eng.packet_init_download()


def differences(grid, ref, pk, dl, keep) -> dict:
    """assert what has to be bit for bit; return the worst rounding ratios in units of 2^-53 (module docstring)"""
    want = ref["packets"]
    for f in DISCRETE:
        assert np.array_equal(pk[f][keep], want[f][keep]), f
    assert np.array_equal(dl["channel"][keep], ref["channel"][keep]) and np.array_equal(dl["trials"][keep], ref["trials"][keep])
    for f in EXACT:
        assert pk[f][keep].tobytes() == want[f][keep].tobytes(), f
    assert np.all(np.isnan(pk["em_pos"])) and np.all(np.isnan(pk["trueem_pos"]))
    paths = keep & (ref["tdecay_unit"] > 0)
    out = dict(tdecay=float(np.max(np.abs(pk["tdecay"][paths] - want["tdecay"][paths]) / ref["tdecay_unit"][paths], initial=0.0)) / U)
    assert pk["tdecay"][keep & ~paths].tobytes() == want["tdecay"][keep & ~paths].tobytes()
    if grid == "3d":
        for f in ("pos", "dir", "e_rf"):
            assert pk[f][keep].tobytes() == want[f][keep].tobytes(), f
        out.update(pos=0.0, dir=0.0, e_rf=0.0)
    else:
        r = np.sqrt(np.sum(want["pos"] ** 2, axis=1))
        out["pos"] = float(np.max(np.abs(pk["pos"] - want["pos"])[keep] / r[keep, None])) / U
        out["dir"] = float(np.max(np.abs(pk["dir"] - want["dir"])[keep])) / U
        out["e_rf"] = float(np.max(np.abs(pk["e_rf"] / want["e_rf"] - 1.0)[keep])) / U
    return out


def check_population(grid, ref, cells, pk, dl, npackets):
    keep = ~undecided(ref)[:npackets]
    assert np.count_nonzero(~keep) <= 2
    assert dl["en_cumulative"].tobytes() == cells["en_cumulative"].tobytes() and dl["endecay_per_mass"].tobytes() == cells["endecay_per_mass"].tobytes()
    assert dl["etot_simtime"] == ref["etot_simtime"] and dl["e_cmf_per_packet"] == ref["e_cmf_per_packet"]
    assert dl["e_cmf_total"] == ref["e_cmf_total"] and dl["e_ratio"] == ref["e_ratio"]
    d = differences(grid, ref, pk, dl, keep)
    print(f"{grid}: worst device - x86 in 2^-53: tdecay {d['tdecay']:.2f} (allowed {ULP_TDECAY}), pos {d['pos']:.2f} ({ULP_POS}), dir {d['dir']:.2f} ({ULP_DIR}), "
          f"e_rf {d['e_rf']:.2f} ({ULP_ERF}); {np.count_nonzero(~keep)} undecided")
    assert d["tdecay"] <= ULP_TDECAY and d["pos"] <= ULP_POS and d["dir"] <= ULP_DIR and d["e_rf"] <= ULP_ERF, d
    assert dl["max_trials"] == int(ref["trials"].max()) or np.count_nonzero(~keep)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_population_is_the_x86_builds(engine_mod, case):
    """20 000 packets with the host's energy vector handed in; the cell of synth.decay_model's zero_cell receives no pellet; a second
    call with the same arguments gives the same bytes (the stage keeps no state between calls)"""
    grid, kind, initial = case
    E, cells, ref = host_reference(*case)
    eng = make_engine(engine_mod, *case)
    info = eng.packet_init(NPK, pc.SEED_BASE, energy_vector=E)
    pk, dl = download(eng, NPK)
    assert dl["energy_vector"].tobytes() == E.tobytes() and info["npackets"] == NPK
    # (the medium network has mean lives of years: a few of its packets need more than one launch's 4096 trials)
    assert dl["continuation_launches"] == -(-int(ref["trials"].max()) // 4096) - 1 and (kind != "small" or dl["continuation_launches"] == 0)
    assert dl["ncheckpoints"] == -(-len(E) // pc.stride())
    check_population(grid, ref, cells, pk, dl, NPK)
    model = pc.case(GRIDS[grid], kind, initial)[0]
    assert not np.any(pk["cellindex"] == pc.propcell_of(model, pc.ZERO_CELL % int(model["npts_nonempty"])))
    assert np.all(np.asarray(model["propcell_nonemptymgi"])[pk["cellindex"]] >= 0)
    if initial:
        assert np.count_nonzero(dl["channel"] == len(E)) > 100
    eng.packet_init(NPK, pc.SEED_BASE, energy_vector=E)
    pk2, dl2 = download(eng, NPK)
    assert pk2.tobytes() == pk.tobytes() and dl2["channel"].tobytes() == dl["channel"].tobytes() and dl2["trials"].tobytes() == dl["trials"].tobytes()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("npackets", [1, 63, 65, 127])
def test_small_populations(engine_mod, npackets):
    """less than a wave, one more than a wave, two waves less one: e_cmf_per_packet and the normalisation change with npackets, the draws
    do not"""
    case = ("3d", "medium", False)
    model, cs, ts, dm, em, pm = pc.case(GRIDS[case[0]], case[1], case[2])
    E, cells, _ = host_reference(*case)
    h = pc.HostPinit(dm, em, pm, model)
    h.cells(E)
    ref = h.run(npackets, margins=True)
    eng = make_engine(engine_mod, *case)
    eng.packet_init(npackets, pc.SEED_BASE, energy_vector=E)
    pk, dl = download(eng, npackets)
    check_population(case[0], ref, cells, pk, dl, npackets)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,initial", [("small", True), ("medium", False)])
def test_own_energy_vector_within_the_bateman_bound(engine_mod, kind, initial):
    """Without a vector handed in the device forms its own: per path |device - x86| <= the Bateman sums' bound of
    tests/test_gpu_decay_update.py at both times, 4 (L + x_dom) 2^-52 scale each, times the exact factors, plus 8 2^-52 of the
    value for the factors' roundings; and the population made from it is the x86 build's for the device's vector."""
    model, cs, ts, dm, em, pm = pc.case(GRIDS["3d"], kind, initial)
    E, cells, ref = host_reference("3d", kind, initial)
    eng = make_engine(engine_mod, "3d", kind, initial)
    eng.packet_init(NPK, pc.SEED_BASE)
    pk, dl = download(eng, NPK)
    net = dm
    L = np.diff(net["path_start"]).astype(np.float64)
    t0 = dc.T_MODEL if initial else float(model["tmin"])
    worst = 0.0
    for p in range(len(E)):
        nuc = net["path_nucindex"][net["path_start"][p]: net["path_start"][p + 1]]
        lam = dc.path_lambdas(net, p)
        lam[-1] = 0.0
        bar = 0.0
        for t in (pc.TMAX - dc.T_MODEL, t0 - dc.T_MODEL):
            _, scale, x = dc.decaychain(lam, t)
            bar += 4 * (L[p] + x) * dc.EPS * scale
        last = nuc[-2]
        factor = float(net["path_branchproduct"][p]) * (em["nuc_endecay_gamma"][last] + np.asarray(em["nuc_endecay_particle"]).reshape(-1, 6)[last, net["path_last_decaytype"][p]]) \
            / pm["nuc_decay_daughters_probsum"][last] / (float(net["nuc_a"][nuc[0]]) * 1.67352e-24)
        bound = bar * factor + 8 * dc.EPS * E[p]
        diff = abs(dl["energy_vector"][p] - E[p])
        assert diff <= bound, (p, diff, bound)
        worst = max(worst, diff / bound if bound > 0 else 0.0)
    print(f"worst |device - x86| / bound of the energy vector = {worst:.4f}")
    h = pc.HostPinit(dm, em, pm, model)
    own_cells = h.cells(dl["energy_vector"])
    own = h.run(NPK, margins=True)
    check_population("3d", own, own_cells, pk, dl, NPK)
    eng.close()


def slow_case(life_factor: float):
    """the 3D small case with the top nuclide of path 0 (a one-decay path) made long-lived: the path accepts a trial in about
    (tmax - tmin) / meanlife of them. (model, dm, em, pm, E): in the energy vector handed in, path 0 gets a tenth of the largest entry,
    so that a good share of the packets draws it although little of the nuclide decays and the cells hold little of it."""
    model, cs, ts, dm0, em, pm = pc.case(GRIDS["3d"], "small", False)
    dm = dict(dm0)
    assert dm["path_start"][1] == 2
    life = np.array(dm["nuc_meanlife"], np.float64)
    life[dm["path_nucindex"][0]] = life_factor * pc.TMAX
    dm["nuc_meanlife"] = life
    E = pc.HostPinit(dm, em, pm, model).energy()
    n = int(model["npts_nonempty"])
    X = np.asarray(dm["initnucmassfrac"], np.float64).reshape(n, -1)
    top = np.asarray(dm["path_nucindex"])[np.asarray(dm["path_start"])[:-1]]
    E[0] = 0.0
    E[0] = 0.25 * float(np.median((X[:, top] @ E)[X[:, top[0]] > 0] / X[:, top[0]][X[:, top[0]] > 0]))  # a fifth of a typical cell's sum
    return model, dm, em, pm, E


@pytest.mark.gpu
def test_continuation_launches_change_nothing(engine_mod):
    """A path with a mean life of 1e3 tmax and a budget of 8 trials per launch: the call needs continuation launches, and its packets,
    generator states and trial counts are those of the default budget (and the x86 build's)."""
    model, dm, em, pm, E = slow_case(1e3)
    npackets = 4000
    h = pc.HostPinit(dm, em, pm, model)
    cells = h.cells(E)
    ref = h.run(npackets, margins=True)
    slow = ref["channel"] == 0
    assert np.count_nonzero(slow) > 20 and ref["trials"][slow].max() > 1000 and not undecided(ref).any()
    out = []
    for budget in (8, 0):
        eng = engine_mod.Engine(model)
        eng.decay_setup(dm)
        eng.deposition_setup(em)
        eng.packet_init_setup({**pm, "max_trials_per_launch": budget})
        eng.packet_init(npackets, pc.SEED_BASE, energy_vector=E)
        out.append(download(eng, npackets))
        eng.close()
    (pk8, dl8), (pk0, dl0) = out
    assert dl8["continuation_launches"] == -(-int(ref["trials"].max()) // 8) - 1 > 100
    assert dl0["continuation_launches"] == -(-int(ref["trials"].max()) // 4096) - 1
    assert pk8.tobytes() == pk0.tobytes() and dl8["channel"].tobytes() == dl0["channel"].tobytes() and dl8["trials"].tobytes() == dl0["trials"].tobytes()
    assert dl8["max_trials"] == dl0["max_trials"] == ref["trials"].max()
    check_population("3d", ref, cells, pk8, dl8, npackets)


@pytest.mark.gpu
def test_a_path_that_cannot_accept_is_refused_and_the_population_stays(engine_mod):
    model, dm, em, pm, E = slow_case(1e12)
    eng = engine_mod.Engine(model)
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    rng = np.random.default_rng(5)
    before = np.zeros(300, abi.PACKET_DTYPE)
    before["type"] = abi.TYPE_ESCAPE
    before["e_cmf"] = rng.random(300)
    before["number"] = np.arange(300)
    eng.upload_packets(before)
    eng.packet_init_setup({**pm, "max_trials_per_launch": 2})
    with pytest.raises(engine_mod.EngineError, match=r"artis_amd error -5: packet_init: path \d+: no decay time"):
        eng.packet_init(500, pc.SEED_BASE, energy_vector=E)
    after = np.zeros(300, abi.PACKET_DTYPE)
    eng.download_packets(after)
    assert after.tobytes() == before.tobytes()
    with pytest.raises(engine_mod.EngineError, match="nothing made"):
        eng.packet_init_download()
    eng.close()


def _step(eng, model, cs, ts0, npackets):
    eng.set_cellstate(cs, ts0)
    eng.zero_estimators()
    eng.step()
    out = np.zeros(npackets, abi.PACKET_DTYPE)
    eng.download_packets(out)
    est = abi.estimators_for(model)
    eng.download_estimators(est)
    return out, est


@pytest.mark.gpu
def test_installed_population_propagates_as_an_uploaded_one(engine_mod):
    """After packet_init the pellets are downloaded and uploaded into a second engine, and both make one step at nts = 0 (from tmin).
    20 000 packets: packets (generator states included) and counters bit-identical; the estimators are sums of device-wide f64
    atomics of many packets per cell, whose order differs between any two runs of the SAME engine, so there they are held to the bar
    of tests/test_gpu_decay_update.py between two runs of the same packets. One packet at a time (eight seeds), where every estimator
    entry has one writer: packets, counters AND estimators bit-identical. A snapshot taken before packet_init is gone after it."""
    case = ("3d", "small", True)
    model, cs, ts, dm, em, pm = pc.case(GRIDS["3d"], "small", True)
    E, cells, ref = host_reference(*case)
    ts0 = synth.make_timestep(float(model["tmin"]), width_frac=1.0, nts=0)
    a = make_engine(engine_mod, *case)
    b = engine_mod.Engine(model)
    old = synth.make_packets(model, pc.grid(GRIDS["3d"])[3], 1000)
    a.upload_packets(old)
    a.snapshot()
    a.packet_init(NPK, pc.SEED_BASE, energy_vector=E)
    with pytest.raises(engine_mod.EngineError, match="no snapshot"):
        a.restore()
    pk, _ = download(a, NPK)
    b.upload_packets(pk)
    (pa, ea), (pb, eb) = _step(a, model, cs, ts0, NPK), _step(b, model, cs, ts0, NPK)
    assert np.count_nonzero(pa["type"] != abi.TYPE_RADIOACTIVE_PELLET) > NPK // 100  # pellets decayed in the step
    assert pa.tobytes() == pb.tobytes() and ea.stats_dict() == eb.stats_dict()
    for k, va in ea.arrays().items():
        if va is None:
            continue
        va, vb = np.asarray(va), np.asarray(eb.arrays()[k])
        assert np.array_equal(va == 0, vb == 0) and np.all(np.abs(va - vb) <= 1e-12 * np.abs(va)), k
    ts1 = synth.make_timestep(float(model["tmin"]), width_frac=30.0, nts=0)  # (a step long enough for most pellets to decay in it)
    moved = nonzero = 0
    for seed in range(8):
        a.packet_init(1, pc.SEED_BASE + seed, energy_vector=E)
        one, _ = download(a, 1)
        b.upload_packets(one)
        (pa, ea), (pb, eb) = _step(a, model, cs, ts1, 1), _step(b, model, cs, ts1, 1)
        assert pa.tobytes() == pb.tobytes() and ea.stats_dict() == eb.stats_dict()
        for k, va in ea.arrays().items():
            if va is None:
                continue
            assert np.asarray(va).tobytes() == np.asarray(eb.arrays()[k]).tobytes(), (seed, k)
            nonzero += int(np.count_nonzero(va))
        moved += int(pa["type"][0] != abi.TYPE_RADIOACTIVE_PELLET)
    assert moved >= 3 and nonzero > 0
    a.close()
    b.close()


@pytest.mark.gpu
def test_refusals_of_the_entry_points(engine_mod):
    model, cs, ts, dm, em, pm = pc.case(GRIDS["3d"], "small", True)
    eng = engine_mod.Engine(model)

    def refused(code, text, f, *args, **kw):
        with pytest.raises(engine_mod.EngineError, match=rf"artis_amd error {code}: packet_init: .*{text}"):
            f(*args, **kw)

    refused(-3, "no network", eng.packet_init_setup, pm)
    eng.decay_setup(dm)
    refused(-3, "no energies", eng.packet_init_setup, pm)
    eng.deposition_setup(em)
    refused(-3, "no set-up", eng.packet_init, 10, 1)
    refused(-4, "UNIFORM_PELLET_ENERGIES", eng.packet_init_setup, {**pm, "uniform_pellet_energies": 0})
    refused(-3, "tmax <= tmin", eng.packet_init_setup, {**pm, "tmax": float(model["tmin"])})
    probsum = np.array(pm["nuc_decay_daughters_probsum"])
    probsum[0] = 0.0
    refused(-3, "nuclide 0: it decays", eng.packet_init_setup, {**pm, "nuc_decay_daughters_probsum": probsum})
    late = dict(dm)
    late["t_model"] = 1.5 * float(model["tmin"])
    eng.decay_setup(late)
    eng.deposition_setup(em)
    refused(-3, "t_model > tmin", eng.packet_init_setup, pm)
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    eng.packet_init_setup(pm)
    refused(-3, "npackets", eng.packet_init, 0, 1)
    bad = np.ones(len(dm["path_start"]) - 1)
    bad[2] = np.nan
    refused(-3, "energy_vector: path 2", eng.packet_init, 10, 1, energy_vector=bad)
    eng.packet_init_setup(pc.case(GRIDS["3d"], "small", False)[5])  # without the initial energy a vector of zeros leaves no energy at all
    refused(-3, "etot_simtime is not positive", eng.packet_init, 10, 1, energy_vector=np.zeros(len(bad)))
    eng.packet_init_setup(pm)
    eng.packet_init(10, 1)
    eng.deposition_setup(em)  # a new deposition set-up invalidates the pellet set-up
    refused(-3, "no set-up", eng.packet_init, 10, 1)
    eng.packet_init_setup(pm)
    eng.decay_setup(dm)  # ... and so does a new decay set-up (with the deposition set-up)
    refused(-3, "no set-up", eng.packet_init, 10, 1)
    eng.close()
