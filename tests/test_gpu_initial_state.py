"""The initial temperatures, grey opacity and first cell state on the device (artis_amd_initial_state*, artis_amd_grid_update_initial)
against the x86 build of the same rules (tests/initial_state_host): with the host's energy vector handed in the cell sums, flags,
counts, thickness and the table opacities bit for bit and T_initial within one float ulp (the device's pow against glibc's); the
device's own vector to the expansion sum's rounding bound; the hand-over on an engine that never saw a cell state against the existing
path fed with the downloaded arrays; a whole first step from the model alone against one from uploaded packets and host arrays; and the
refusals.

The non-finite branch is reached with finite inputs (initial_common.four_branches): the set-ups refuse an infinite initenergyq,
rho_tmin or vector entry, so one cell gets an energy per mass of 1.7e308, whose product under the root overflows."""
import ctypes as C

import numpy as np
import pytest

import initial_common as ic
import packet_init_common as pc
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
NPK = 20000
# (grid, network, initial-energy channel, preset, grey type): 5, 56 and 280 = 4 x 64 + 24 non-empty cells; 20 paths (fewer than
# CKPT_DEPTH), 196 = 6 x 32 + 4 and 2100 = 65 x 32 + 20 paths
CASES = [("1d", "small", True, "classic", abi.GREY_FEGROUP_APPROX), ("3d", "medium", False, "classic", abi.GREY_TANAKA2020),
         ("2d", "small", True, "kilonova_lte", abi.GREY_JUST2022), ("3d", "small20", False, "kilonova_lte", abi.GREY_TANAKA2020),
         ("3d", "medium", True, "kilonova_lte", abi.GREY_JUST2022)]
IDS = ["-".join(map(str, c)) for c in CASES]


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def make_engine(engine_mod, model, dm, em, pm, preset):
    eng = engine_mod.Engine(model, preset=preset)
    eng.decay_setup(dm)
    eng.deposition_setup(em)
    eng.packet_init_setup(pm)
    return eng


def depth_threshold(host, params, E, dec, Z):
    """an optical depth that about half of the cells exceed and none comes near (4 float ulps)"""
    depth = np.sort(host.cells(params, E, dec["rho"], dec["elem_massfracs"], Z)["grey_depth"].astype(np.float64))
    mid = len(depth) // 2
    cut = 0.5 * (depth[mid - 1] + depth[mid]) if len(depth) > 1 and depth[mid] > depth[mid - 1] else 0.5 * depth[mid]
    assert np.all(np.abs(depth - cut) > 8 * np.spacing(np.float32(cut)))
    return float(cut)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cells_are_the_x86_builds_with_the_hosts_vector(engine_mod, case):
    grid, kind, channel, preset, grey = case
    model, cs, dm0, em, pm0 = ic.case(grid, kind, channel, preset)
    params = ic.step_params(model, cs, grey)
    E0 = ic.HostInitial(dm0, em, pm0, model, preset).energy(params["tstart"])["energy_vector"]
    dm, pm, E = ic.four_branches(dm0, pm0, model, E0, preset)
    host = ic.HostInitial(dm, em, pm, model, preset)
    Z = np.asarray(model["elem_anumber"], np.int32)
    eng = make_engine(engine_mod, model, dm, em, pm, preset)
    dec = eng.decay_update(params["tstart"])
    params["optical_depth_is_thick"] = depth_threshold(host, params, E, dec, Z)
    params["optical_depth_is_thick_vpkt"] = 0.5 * params["optical_depth_is_thick"]
    d = eng.initial_state(dict(params, energy_vector=E))
    want = host.cells(params, E, dec["rho"], dec["elem_massfracs"], Z)
    n = int(model["npts_nonempty"])
    assert d["energy_vector"].tobytes() == E.tobytes() and not d["path_scale"].any() and d["npts_nonempty"] == n and d["tstart"] == params["tstart"]
    assert d["endecay_per_mass"].tobytes() == want["endecay_per_mass"].tobytes()
    assert np.array_equal(d["flags"], want["flags"]) and d["ncells_branch"] == want["ncells_branch"] and d["ncells_kappa_invalid"] == 0
    assert all(v >= 1 for v in d["ncells_branch"].values()) and sum(d["ncells_branch"].values()) == n
    bad = ic.NONFINITE_CELL % n
    assert d["first_nonfinite_cell"] == want["first_nonfinite_cell"] == bad
    assert d["first_nonfinite_rho_tmin"] == float(np.float32(dm["rho_tmin"][bad])) and d["first_nonfinite_endecay"] == want["endecay_per_mass"][bad]
    uT = _ulps(d["T_initial"], want["T_initial"])
    assert uT.max() <= 1, int(uT.max())
    own = host.grey(params, dec["rho"], dec["elem_massfracs"], Z, d["T_initial"])  # the x86 rules from the device's own T_initial
    if grey == abi.GREY_JUST2022:
        assert _ulps(d["kappagrey"], own["kappagrey"]).max() <= 1
        assert np.any(d["T_initial"] < 2000.0) and np.any(d["T_initial"] > 2000.0) and len(set(d["kappagrey"])) > 1
    else:
        assert d["kappagrey"].tobytes() == want["kappagrey"].tobytes() == own["kappagrey"].tobytes()
    assert _ulps(d["grey_depth"], own["grey_depth"]).max() <= 1
    assert np.array_equal(d["thick"], own["thick"]) and (grey == abi.GREY_JUST2022 or np.array_equal(d["thick"], want["thick"]))
    assert 0 < np.count_nonzero(d["thick"] == abi.CELL_THICK) < n
    print(f"{IDS[CASES.index(case)]}: {int((uT == 1).sum())} of {n} T_initial one ulp apart, branches {d['ncells_branch']}, kernels {d['kernel_ms']}")
    # a second call gives the same bytes (the stage keeps no state between calls)
    d2 = eng.initial_state(dict(params, energy_vector=E))
    for k in ("T_initial", "endecay_per_mass", "kappagrey", "grey_depth", "thick", "flags"):
        assert d2[k].tobytes() == d[k].tobytes(), k
    eng.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_own_energy_vector_within_the_expansion_sums_bound(engine_mod, case):
    """Without a vector handed in the device forms its own: per path |device - x86| <= 4 (L + x_dom) 2^-52 scale x the exact
    factors, with the scale of the summands before their cancellation; T_initial within that bound propagated through the cell's sum,
    1/4 sum X bound / sum X E relative, plus one float ulp"""
    grid, kind, channel, preset, grey = case
    model, cs, dm, em, pm = ic.case(grid, kind, channel, preset)
    params = ic.step_params(model, cs, grey)
    host = ic.HostInitial(dm, em, pm, model, preset)
    x86 = host.energy(params["tstart"])
    eng = make_engine(engine_mod, model, dm, em, pm, preset)
    dec = eng.decay_update(params["tstart"])
    d = eng.initial_state(params)
    bound = ic.energy_bound(dm, em, pm, x86["path_scale"], x86["path_x_dom"])
    diff = np.abs(d["energy_vector"] - x86["energy_vector"])
    assert np.all(diff <= bound), (int(np.argmax(diff - bound)), float(np.max(diff - bound)))
    assert np.array_equal(d["path_x_dom"], x86["path_x_dom"]) and np.all(np.abs(d["path_scale"] - x86["path_scale"]) <= 8 * ic.EPS * x86["path_scale"])
    assert np.count_nonzero(d["energy_vector"]) > len(bound) // 2
    print(f"{kind}: worst |device - x86| / bound of the energy vector = {float(np.max(diff[bound > 0] / bound[bound > 0], initial=0.0)):.4f}")
    Z = np.asarray(model["elem_anumber"], np.int32)
    want = host.cells(params, x86["energy_vector"], dec["rho"], dec["elem_massfracs"], Z)
    n, nn = int(model["npts_nonempty"]), len(dm["nuc_z"])
    X = np.asarray(dm["initnucmassfrac"], np.float64).reshape(n, nn)
    top = np.asarray(dm["path_nucindex"])[np.asarray(dm["path_start"])[:-1]]
    e = want["endecay_per_mass"]
    rel = np.where(e > 0, 0.25 * (X[:, top] @ bound) / np.where(e > 0, e, 1.0), 0.0)
    both_inside = ((d["flags"] | want["flags"]) & abi.INITIAL_BRANCH_MASK) == abi.INITIAL_INSIDE
    assert np.count_nonzero(both_inside) > n // 2
    T = want["T_initial"].astype(np.float64)
    assert np.all(np.abs(d["T_initial"].astype(np.float64) - T)[both_inside] <= (T * rel + np.spacing(want["T_initial"]))[both_inside])
    # and the cells are the x86 build's for the device's own vector
    again = host.cells(params, d["energy_vector"], dec["rho"], dec["elem_massfracs"], Z)
    assert d["endecay_per_mass"].tobytes() == again["endecay_per_mass"].tobytes() and _ulps(d["T_initial"], again["T_initial"]).max() <= 1
    eng.close()


def seed_cellstate(model, cs, dec, preset):
    """what the reference holds before its first update_grid, as an artis_cellstate: ground populations of 0, W = 1, THICK flags,
    corrphotoionrenorm 1 (grid.cc:427, :561, update_grid.cc:495-501)"""
    n, ni, g = int(model["npts_nonempty"]), int(model["nions"]), max(int(model["nbfcontinua_ground"]), 1)
    s = dict(cs.d)
    s.update(ion_groundlevelpops=np.zeros(n * ni, np.float32), W=np.ones(n, np.float32),
             thick=np.full(n, abi.CELL_THICK, np.int32), corrphotoionrenorm=np.ones(n * g), clumpfactor=np.ones(n, np.float32))
    if ic.calculated_meanweight(preset):
        s["elem_meanweight"] = dec["elem_meanweight"].ravel()
    return abi.CellState(s)


def first_state_two_ways(engine_mod, grid, kind, channel, preset, grey, with_packets=0):
    """engine A: from the model alone; engine B: the existing path fed with A's downloaded arrays. Returns (A, B, A's and B's downloads)"""
    model, cs, dm, em, pm = ic.case(grid, kind, channel, preset)
    ts0 = ic.first_timestep(model)
    params = ic.step_params(model, cs, grey)
    assert params["tstart"] == ts0.c.mid
    Z = np.asarray(model["elem_anumber"], np.int32)
    n = int(model["npts_nonempty"])
    ones, ffegrp = np.ones(n, np.float32), np.asarray(cs["ffegrp"], np.float32)
    a = make_engine(engine_mod, model, dm, em, pm, preset)
    if with_packets:
        a.packet_init(with_packets, pc.SEED_BASE)
    dec = a.decay_update(params["tstart"])
    host = ic.HostInitial(dm, em, pm, model, preset)
    params["optical_depth_is_thick"] = depth_threshold(host, params, host.energy(params["tstart"])["energy_vector"], dec, Z)
    init = a.initial_state(params)
    assert 0 < np.count_nonzero(init["thick"] == abi.CELL_THICK) < n
    da = a.grid_update_initial(ts0, clumpfactor=ones, ffegrp=ffegrp)
    b = engine_mod.Engine(model, preset=preset)
    b.set_cellstate(seed_cellstate(model, cs, dec, preset), ts0)
    T = init["T_initial"]
    db = b.grid_update(ts0, dec["rho"], dec["elem_massfracs"].ravel(), init["thick"], use_fit=False,
                       elem_meanweight=dec["elem_meanweight"].ravel() if ic.calculated_meanweight(preset) else None, TJ=T, TR=T, W=ones, Te=T,
                       kappagrey=init["kappagrey"], clumpfactor=ones, ffegrp=ffegrp)
    return model, a, b, da, db, init


XCOM_CASE = ("3d", "small", False, "ci_kilonova_xcom", abi.GREY_TANAKA2020)  # USE_CALCULATED_MEANATOMICWEIGHT and USE_XCOM_GAMMAPHOTOION:
# a cell state without elem_meanweight is refused there, so the first state has to have the array before the options are checked


@pytest.mark.parametrize("case", [CASES[1], CASES[2], XCOM_CASE], ids=[IDS[1], IDS[2], "-".join(map(str, XCOM_CASE))])
def test_handover_without_a_resident_cell_state(engine_mod, case):
    """everything artis_amd_grid_update_download returns and the cell cache of three cells, bit for bit against the existing path"""
    model, a, b, da, db, init = first_state_two_ways(engine_mod, *case)
    for k, va in da.items():
        if isinstance(va, np.ndarray):
            assert va.tobytes() == db[k].tobytes(), k
    assert da["ncells_flagged"] == db["ncells_flagged"] and da["total_evals"] == db["total_evals"]
    n = int(model["npts_nonempty"])
    assert da["ncells_flagged"]["forced_saha"] == n and np.all(da["W"] == 1.0) and da["TJ"].tobytes() == init["T_initial"].tobytes() == da["Te"].tobytes()
    assert np.count_nonzero(da["ion_groundlevelpops"]) > 0
    for c in (0, n // 2, n - 1):
        ca, cb = a.debug_cellcache(c), b.debug_cellcache(c)
        for k, va in ca.items():
            assert np.asarray(va).tobytes() == np.asarray(cb[k]).tobytes(), (c, k)
    # a second initial call on the now resident state gives the same state
    ones = np.ones(n, np.float32)
    da2 = a.grid_update_initial(ic.first_timestep(model), clumpfactor=ones, ffegrp=np.asarray(ic.case(*case[:4])[1]["ffegrp"], np.float32))
    for k in ("Te", "nne", "ion_groundlevelpops", "ion_partfuncts", "flags"):
        assert da2[k].tobytes() == da[k].tobytes(), k
    a.close()
    b.close()


def test_first_step_from_the_model_alone(engine_mod):
    """Engine A: packet_init -> decay_update(tstart) -> initial_state -> grid_update_initial -> one propagation step, no per-cell array
    from the host. Engine B: the same packets uploaded, the first state by the existing path. Packets, generator states and counters
    bit for bit; the estimators to the 1e-12 bar of tests/test_gpu_packet_init.py between two runs (the order of f64 atomics)."""
    model, a, b, da, db, init = first_state_two_ways(engine_mod, "3d", "small", True, "classic", abi.GREY_FEGROUP_APPROX, with_packets=NPK)
    pk = np.zeros(NPK, abi.PACKET_DTYPE)
    a.download_packets(pk)
    b.upload_packets(pk)
    outs = []
    for eng in (a, b):
        eng.zero_estimators()
        eng.step()
        out = np.zeros(NPK, abi.PACKET_DTYPE)
        eng.download_packets(out)
        est = abi.estimators_for(model)
        eng.download_estimators(est)
        outs.append((out, est))
    (pa, ea), (pb, eb) = outs
    assert np.count_nonzero(pa["type"] != abi.TYPE_RADIOACTIVE_PELLET) > 0  # pellets decayed in the step
    assert pa.tobytes() == pb.tobytes() and ea.stats_dict() == eb.stats_dict()
    for k, va in ea.arrays().items():
        if va is None:
            continue
        va, vb = np.asarray(va), np.asarray(eb.arrays()[k])
        assert np.array_equal(va == 0, vb == 0) and np.all(np.abs(va - vb) <= 1e-12 * np.abs(va)), k
    a.close()
    b.close()


def test_refusals(engine_mod):
    model, cs, dm, em, pm = ic.case("3d", "small", True, "classic")
    ts0 = ic.first_timestep(model)
    params = ic.step_params(model, cs, abi.GREY_FEGROUP_APPROX)
    n = int(model["npts_nonempty"])
    ones = np.ones(n, np.float32)
    eng = engine_mod.Engine(model)

    def refused(code, text, f, *args, **kw):
        with pytest.raises(engine_mod.EngineError, match=rf"artis_amd error {code}: .*{text}"):
            f(*args, **kw)

    refused(-3, "initial_state: no network", eng.initial_state, params)
    eng.decay_setup(dm)
    refused(-3, "initial_state: no energies", eng.initial_state, params)
    eng.deposition_setup(em)
    refused(-3, "initial_state: no pellet set-up", eng.initial_state, params)
    eng.packet_init_setup(pm)
    refused(-3, "initial_state: no decay update at t_mid == tstart", eng.initial_state, params)
    refused(-3, "grid_update_initial: no initial state", eng.grid_update_initial, ts0, clumpfactor=ones)
    eng.decay_update(params["tstart"])
    refused(-3, "tstart < t_model", eng.initial_state, dict(params, tstart=0.5 * ic.T_MODEL))
    refused(-3, "unknown rpkt_grey_type 7", eng.initial_state, dict(params, rpkt_grey_type=7))
    ye = np.array(params["initelectronfrac"])
    ye[4] = -0.1
    refused(-3, "cell 4: TANAKA2020 with Ye <= 0", eng.initial_state, dict(params, rpkt_grey_type=abi.GREY_TANAKA2020, initelectronfrac=ye))
    bad = np.ones(len(dm["path_start"]) - 1)
    bad[2] = np.nan
    refused(-3, "energy_vector: path 2", eng.initial_state, dict(params, energy_vector=bad))
    refused(-3, "nothing made", eng.initial_state_download)
    eng.initial_state(params)
    def raw_initial(use_fit, **arrays):  # the struct as a caller could fill it, past the Python method that fills it rightly
        u, keep = abi.grid_update_config(use_fit, None, None, None, clumpfactor=ones, **arrays)
        eng._check(eng.L.artis_amd_grid_update_initial(eng.h, C.byref(u), C.cast(ts0.ref(), C.c_void_p), None))

    refused(-3, "use_fit must be 0", raw_initial, True)
    refused(-3, "must be NULL", raw_initial, False, Te=ones)
    refused(-3, "clumpfactor is required", eng.grid_update_initial, ts0)
    refused(-3, "another nts", eng.grid_update_initial, synth.make_timestep(float(model["tmin"]), width_frac=0.05, vmax=float(model["vmax"]), nts=1), clumpfactor=ones)
    eng.decay_update(1.5 * params["tstart"])  # a decay update at another t_mid
    refused(-3, "not made on the decay update of ts_first", eng.grid_update_initial, ts0, clumpfactor=ones)
    eng.decay_update(params["tstart"])  # ... and the same t_mid again is still another update than the one the state was made on
    refused(-3, "not made on the decay update of ts_first", eng.grid_update_initial, ts0, clumpfactor=ones)
    eng.initial_state(params)
    eng.grid_update_initial(ts0, clumpfactor=ones)
    eng.decay_setup(dm)  # a new network: the initial state is no longer one of it
    refused(-3, "no initial state", eng.grid_update_initial, ts0, clumpfactor=ones)
    eng.close()
    # the nebular family
    nmodel, ncs, nts, naux = synth.build("small", ncoord=6, options="nltenebular")
    e3 = engine_mod.Engine(synth.with_meannucmass(nmodel), preset="nltenebular")
    refused(-4, "initial_state: this build has NLTE populations", e3.initial_state, params)
    refused(-4, "grid_update_initial: this build has NLTE populations", e3.grid_update_initial, ts0, clumpfactor=ones)
    e3.close()


def test_a_refused_balance_leaves_no_cell_state(engine_mod):
    """An invalid partition function (a ground level with statistical weight 0: U = 0) refuses the balance of every cell; an engine
    that had no cell state has none afterwards, the flags stay downloadable, and a propagation call answers as before any state."""
    model, cs, dm, em, pm = ic.case("1d", "small", False, "classic")
    md = dict(model.d)
    md["level_statweight"] = np.array(md["level_statweight"], np.float32)
    md["level_statweight"][0] = 0.0
    bad_model = abi.Model(md)
    params = ic.step_params(model, cs, abi.GREY_FEGROUP_APPROX)
    n = int(model["npts_nonempty"])
    eng = make_engine(engine_mod, bad_model, dm, em, pm, "classic")
    eng.packet_init(500, pc.SEED_BASE)
    eng.decay_update(params["tstart"])
    eng.initial_state(params)
    with pytest.raises(engine_mod.EngineError, match=r"artis_amd error -5: grid_update: \d+ cells .*invalid partition function"):
        eng.grid_update_initial(ic.first_timestep(model), clumpfactor=np.ones(n, np.float32))
    d = eng.grid_update_download()
    assert d["ncells_flagged"]["invalid_u"] == n
    with pytest.raises(engine_mod.EngineError, match="set_cellstate"):
        eng.step()
    with pytest.raises(engine_mod.EngineError):
        eng.debug_cellcache(0)
    eng.close()
