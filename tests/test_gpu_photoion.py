"""The photoionisation coefficients of builds without USE_LUT_PHOTOION on the device (artis_amd_set_cellstate_photoion) against the x86
build of the same rules (tests/photoion_host) with the stage's own exp and expm1: every other operation is +, -, x, / in one order, so
every coefficient, source byte, flag and total must be the same bits on both machines. Then launch and cell boundaries, a model of
three continua, edge cells, the hand-over to the cell state against artis_amd_set_cellstate with the downloaded array and against the
oracle, the fit's estimators device to device, and the refusals. Model: synth "small" on 3 cells per axis (19 non-empty cells x 159
continua) with the options of nltenebular and ci_nebular_limitbfest."""
import ctypes as C

import numpy as np
import pytest

import parity
import photoion_common as pc
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu
NPK = 2000
FLOAT_RTOL = EST_RTOL = 1e-9  # the bars of tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available()
    from artis_amd import engine

    return engine


def _set(eng, model, cells, aux, use_bf=False, bf=None, nts=pc.NTS, **kw):
    eng.set_cellstate_photoion(pc.cellstate(cells), pc.timestep(model, aux, nts), use_bf_estimators=use_bf, bfrate_normed=bf, **kw)
    return eng.photoion()


@pytest.fixture(scope="module", params=pc.PRESETS)
def computed(engine_mod, request):
    """an engine of the preset, the x86 build's view of its model and the seeded estimators (made once, never changed)"""
    preset = request.param
    model, cells, host_corr, aux = pc.state(preset)
    hm = pc.HostModel(model, preset)
    eng = engine_mod.Engine(model, preset=preset)
    yield dict(preset=preset, eng=eng, model=model, cells=cells, aux=aux, hm=hm, bf=pc.seeded_bfrate(hm.n, hm.nbfestim))
    eng.close()


@pytest.mark.parametrize("use_bf", [True, False])
def test_device_matches_x86_bit_for_bit(computed, use_bf):
    hm, bf = computed["hm"], computed["bf"]
    d = _set(computed["eng"], computed["model"], computed["cells"], computed["aux"], use_bf, bf if use_bf else None)
    h = hm.compute(pc.call_inputs(computed["cells"], use_bf, bf))
    print(f"{computed['preset']} estimators {use_bf}: {d['totals']}, kernel {d['kernel_ms']:.3f} ms")
    assert (d["npts_nonempty"], d["nphixstargets_total"], d["nbfcontinua"], d["nbfestim"]) == (hm.n, hm.nentries, hm.ncont, hm.nbfestim)
    pc.same_result(d, h, (computed["preset"], use_bf))
    t = d["totals"]
    assert t["from_estimators"] + t["integrals"] == hm.n * hm.ncont and t["nonfinite"] == 0 and not d["flags"].any()
    assert (t["from_estimators"] > 0) == use_bf and t["nodes"] >= t["integrals"] > 0
    assert np.isfinite(d["coeff"]).all() and (d["coeff"] >= 0).all()
    if use_bf and computed["preset"] == "ci_nebular_limitbfest":  # continua without an estimator: the integral
        assert (d["source"][:, hm.conts[hm.conts[:, 3] < 0, 2]] == pc.SRC_INTEGRAL).all()


def test_launch_and_cell_boundaries(computed):
    """159 continua and 64 lanes: wave boundaries fall inside a cell; 5 and 1 cells per launch are launches of a few workgroups"""
    eng, bf = computed["eng"], computed["bf"]
    args = (eng, computed["model"], computed["cells"], computed["aux"], True, bf)
    whole = _set(*args)
    for per_launch in (5, 1):
        pc.same_result(_set(*args, cells_per_launch=per_launch), whole, (computed["preset"], per_launch))


def test_less_than_one_wave(engine_mod, monkeypatch):
    """a model of one ionising ion of three levels: three continua per cell"""
    monkeypatch.setitem(synth.PRESETS, "one_ion", ([(14, 1, 2)], 3, 1.0, 12))
    model, cs, ts, aux = synth.build("one_ion", ncoord=2, options="nltenebular", nts=pc.NTS)
    cells = {k: v for k, v in cs.d.items() if k != "corrphotoioncoeff"}
    hm = pc.HostModel(model, "nltenebular")
    assert hm.ncont == 3 and hm.n >= 1
    eng = engine_mod.Engine(model, preset="nltenebular")
    d = _set(eng, model, cells, aux)
    eng.close()
    pc.same_result(d, hm.compute(pc.call_inputs(cells)), "one ion")
    assert d["totals"]["integrals"] == 3 * hm.n and (d["coeff"][:, hm.conts[:, 2]] > 0).all()


def test_edge_cells(computed):
    """the edge cells of tests/test_photoion_rules.py on the device, with the multibin field and with the dilute black body"""
    hm, eng, model, aux = computed["hm"], computed["eng"], computed["model"], computed["aux"]
    cells = pc.edge_cells(model, computed["cells"], hm)
    for nts in (pc.NTS, pc.NTS_EARLY):
        d = _set(eng, model, cells, aux, nts=nts)
        pc.same_result(d, hm.compute(pc.call_inputs(cells, nts=nts)), (computed["preset"], "edges", nts))
        assert np.isfinite(d["coeff"]).all() and not d["flags"].any()
        if nts == pc.NTS:
            assert d["coeff"][pc.EDGE_ALL_BINS_EMPTY].tobytes() == bytes(8 * hm.nentries)


def test_nonfinite_refuses_the_state(engine_mod, computed):
    """T_e = NaN in one cell: NOTCONVERGED, the block still downloadable and equal to the x86 build's, and no cell state"""
    hm, model, aux = computed["hm"], computed["model"], computed["aux"]
    cells = pc.edge_cells(model, computed["cells"], hm, bad=True)
    eng = engine_mod.Engine(model, preset=computed["preset"])
    with pytest.raises(engine_mod.EngineError, match=f"error -5.*{hm.ncont} coefficients are not finite"):
        _set(eng, model, cells, aux)
    d = eng.photoion()
    # (the bits of a NaN are the machine's: x86 gives the sign bit set, the device clear; everything that is a number is held to its bits)
    h = hm.compute(pc.call_inputs(cells))
    nan = np.isnan(h["coeff"])
    assert np.array_equal(np.isnan(d["coeff"]), nan) and nan.sum() == hm.ncont and nan[pc.EDGE_TE_NAN, hm.conts[:, 2]].all()
    assert d["coeff"][~nan].tobytes() == h["coeff"][~nan].tobytes()
    assert d["source"].tobytes() == h["source"].tobytes() and d["flags"].tobytes() == h["flags"].tobytes() and d["totals"] == h["totals"]
    assert d["flags"].tolist() == [abi.PHOTOION_NONFINITE if c == pc.EDGE_TE_NAN else 0 for c in range(hm.n)]
    pk = synth.make_packets(model, aux, 100, kpkt_fraction=0.2)
    with pytest.raises(engine_mod.EngineError, match="error -3.*set_cellstate"):
        eng.update_packets(pk, abi.estimators_for(model, computed["preset"]))
    eng.close()


def _step(eng, model, aux, preset):
    pk = synth.make_packets(model, aux, NPK, kpkt_fraction=0.2)
    est = abi.estimators_for(model, preset)
    eng.update_packets(pk, est)
    return pk, est


def test_hand_over(engine_mod, oracle, computed):
    """an engine set through set_cellstate_photoion and one set through set_cellstate with the downloaded coefficients propagate 2000
    packets alike; the oracle, given the downloaded coefficients, agrees within the bars of tests/test_gpu_parity.py"""
    preset, model, cells, aux, hm = (computed[k] for k in ("preset", "model", "cells", "aux", "hm"))
    ts = pc.timestep(model, aux)
    ea, eb = engine_mod.Engine(model, preset=preset), engine_mod.Engine(model, preset=preset)
    d = _set(ea, model, cells, aux, True, computed["bf"])
    cs_b = pc.cellstate(cells, corrphotoioncoeff=d["coeff"].ravel())
    eb.set_cellstate(cs_b, ts)
    (pa, sa), (pb, sb) = _step(ea, model, aux, preset), _step(eb, model, aux, preset)
    for c in (0, 7, hm.n - 1):
        ca, cb = ea.debug_cellcache(c)["corrphotoioncoeff"], eb.debug_cellcache(c)["corrphotoioncoeff"]
        assert ca.tobytes() == cb.tobytes() == d["coeff"][c].tobytes(), c
    ea.close()
    eb.close()
    for f in abi.PACKET_DTYPE.names:  # every field, the generator states among them
        assert pa[f].tobytes() == pb[f].tobytes(), f
    assert np.array_equal(sa.stats, sb.stats) and pa["pos"].tobytes() != synth.make_packets(model, aux, NPK, kpkt_fraction=0.2)["pos"].tobytes()
    po = synth.make_packets(model, aux, NPK, kpkt_fraction=0.2)
    so = abi.estimators_for(model, preset)
    oracle.update_packets(model, cs_b, ts, po, so, preset=preset)
    rep = parity.compare_packets(pa, po, FLOAT_RTOL, preset + ": set_cellstate_photoion vs oracle")
    parity.compare_stats(sa, so, preset + ": set_cellstate_photoion vs oracle", same_libm=False)
    parity.compare_estimators(sa, so, EST_RTOL, preset + ": set_cellstate_photoion vs oracle")
    print(f"worst float rel diff {rep['worst_rel']:.3e}")


def test_fit_to_photoion_device_to_device(engine_mod, computed):
    """after a propagation call and artis_amd_radfield_fit, bfrate_normed = None takes the fit's block where it lies"""
    preset, model, cells, aux, hm = (computed[k] for k in ("preset", "model", "cells", "aux", "hm"))
    ts = pc.timestep(model, aux)
    eng = engine_mod.Engine(model, preset=preset)
    _set(eng, model, cells, aux)
    _step(eng, model, aux, preset)
    fit = eng.radfield_fit(ts.c.mid, ts.c.width, synth.assocvolume_tmin(model))
    bf = fit["bfrate_normed"].reshape(hm.n, hm.nbfestim)
    d = _set(eng, model, cells, aux, True, None, nts=pc.NTS + 1)
    eng.close()
    pc.same_result(d, hm.compute(pc.call_inputs(cells, True, bf, nts=pc.NTS + 1)), (preset, "fit"))
    nest = 0
    for ul, t, entry, bi in hm.conts:
        est = d["source"][:, entry] == pc.SRC_ESTIMATOR
        assert bi >= 0 or not est.any()
        assert d["coeff"][est, entry].tobytes() == bf[est, bi].astype(np.float64).tobytes()
        nest += int(est.sum())
    assert nest == d["totals"]["from_estimators"] > 0


def test_refusals(engine_mod, computed):
    EngineError = engine_mod.EngineError
    preset, model, cells, aux, hm, eng = (computed[k] for k in ("preset", "model", "cells", "aux", "hm", "eng"))
    ts = pc.timestep(model, aux)
    host_corr = pc.state(preset)[2]
    with pytest.raises(EngineError, match="error -3.*corrphotoioncoeff must be NULL"):
        eng.set_cellstate_photoion(pc.cellstate(cells, corrphotoioncoeff=host_corr), ts)
    fresh = engine_mod.Engine(model, preset=preset)
    with pytest.raises(EngineError, match="error -3.*nothing computed"):
        fresh.photoion()
    with pytest.raises(EngineError, match="error -3.*needs a valid artis_amd_radfield_fit"):
        fresh.set_cellstate_photoion(pc.cellstate(cells), ts, use_bf_estimators=True)
    with pytest.raises(EngineError, match="error -3.*levelpops is required"):
        fresh.set_cellstate_photoion(abi.CellState({k: v for k, v in cells.items() if k != "levelpops"}), ts)
    with pytest.raises(EngineError, match="error -3.*radfieldbin_W"):
        fresh.set_cellstate_photoion(abi.CellState({k: v for k, v in cells.items() if k != "radfieldbin_W"}), ts)
    with pytest.raises(EngineError, match="error -3.*cells_per_launch"):
        fresh.set_cellstate_photoion(pc.cellstate(cells), ts, cells_per_launch=-1)
    p = abi.PhotoionParams(struct_size=C.sizeof(abi.PhotoionParams) - 8)
    with pytest.raises(EngineError, match="error -3.*struct_size"):
        fresh._check(fresh.L.artis_amd_set_cellstate_photoion(fresh.h, C.cast(pc.cellstate(cells).ref(), C.c_void_p), C.cast(ts.ref(), C.c_void_p),
                                                              C.byref(p), None))
    # artis_amd_set_cellstate without the array is still refused; and it makes an earlier block stale
    with pytest.raises(EngineError, match="error -3.*corrphotoioncoeff is required"):
        fresh.set_cellstate(pc.cellstate(cells), ts)
    _set(fresh, model, cells, aux)
    fresh.set_cellstate(pc.cellstate(cells, corrphotoioncoeff=host_corr), ts)
    with pytest.raises(EngineError, match="error -3.*nothing computed for the cell state that was set last"):
        fresh.photoion()
    fresh.close()


def test_refusals_of_other_builds(engine_mod):
    """a classic build: use_bf_estimators is refused (no DETAILED_BF_ESTIMATORS_ON), and without it the call is UNSUPPORTED
    (USE_LUT_PHOTOION: the coefficients come from the table)"""
    model, cs, ts, aux = synth.build("small", ncoord=3)
    eng = engine_mod.Engine(synth.with_meannucmass(model))
    with pytest.raises(engine_mod.EngineError, match="error -3.*without DETAILED_BF_ESTIMATORS_ON"):
        eng.set_cellstate_photoion(cs, ts, use_bf_estimators=True)
    with pytest.raises(engine_mod.EngineError, match="error -4.*USE_LUT_PHOTOION"):
        eng.set_cellstate_photoion(cs, ts)
    eng.close()
