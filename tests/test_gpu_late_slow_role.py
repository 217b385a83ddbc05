"""GPU tests of k_late's third role: the slow-path actions -- free-bound emissions, the deferred macro-atom searches -- run
inside the persistent launch on a queue of their own, so that k_late ends the population: no k_slow and no k_tail launch follows it. Where a
packet is advanced is placement: every field of every packet, the generator states and the event counters are those of the split kernels; the
estimators are theirs to summation order. Helpers, tolerances and shapes are those of tests/test_gpu_late_kernel.py; every run sets
ARTIS_AMD_LATE_STRICT=1, which turns a wave of k_late that gave up waiting for work into an error (zero bail-outs in every case here).

The two inputs of the first test give 8 + 71 and 2 + 34 free-bound events (K_STAT_TO_R_FB + MA_STAT_DEACTIVATION_FB) on the CPU oracle."""
import numpy as np
import pytest

import parity
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-9  # packets against the oracle (test_gpu_late_kernel.FLOAT_RTOL)
LATE_VARIABLES = ("ARTIS_AMD_LATE", "ARTIS_AMD_LATE_ALWAYS", "ARTIS_AMD_LATE_STRICT")
NEVER = {"ARTIS_AMD_LATE": "0"}
ALWAYS = {"ARTIS_AMD_LATE": "100000000", "ARTIS_AMD_LATE_ALWAYS": "1"}


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from artis_amd import engine

    engine.load_library()
    return engine


def run(engine_mod, monkeypatch, model, cs, ts, pk0, env, options="classic"):
    """one step of the packets on a new engine created under `env` (+ ARTIS_AMD_LATE_STRICT=1)"""
    for v in LATE_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ARTIS_AMD_LATE_STRICT", "1")
    eng = engine_mod.Engine(model, preset=options)
    eng.set_cellstate(cs, ts)
    p, e = pk0.copy(), abi.estimators_for(model, options)
    eng.update_packets(p, e)
    out = dict(p=p, e=e, kinds=eng.last_kernel_ms_by_kind(), variants=eng.last_thermal_variants())
    eng.close()
    return out


def ran_late(engine_mod, out):
    bit = bool(out["variants"] & engine_mod.Engine.THERMAL_LATE)
    assert bit == (out["kinds"]["k_late"]["launches"] > 0), (out["variants"], out["kinds"])
    return bit


def same(got, want, what):
    parity.compare_packets(got["p"], want["p"], 0.0, what)
    assert np.array_equal(got["p"]["rngstate"], want["p"]["rngstate"]), what
    parity.compare_stats(got["e"], want["e"], what)
    parity.compare_estimators(got["e"], want["e"], 1e-11, what)


def fb_events(out):
    st = out["e"].stats_dict()
    return st["K_STAT_TO_R_FB"] + st["MA_STAT_DEACTIVATION_FB"]


@pytest.mark.parametrize("data,ncoord,npk,kfrac,with_oracle", [("small", 8, 6000, 0.2, True), ("w7", 6, 3000, 0.8, False)])
def test_late_kernel_ends_the_population(engine_mod, oracle, monkeypatch, data, ncoord, npk, kfrac, with_oracle):
    """r-packets and k-packets only (nothing leaves for the gamma-ray kernel): with ARTIS_AMD_LATE_ALWAYS the step is k_late's alone -- no k_slow and
    no k_tail launch -- the free-bound events happened (the slow role and the wave's frequency selection ran), and the results are the split kernels'"""
    model, cs, ts, aux = synth.build(data, ncoord=ncoord)
    pk0 = synth.make_packets(model, aux, npk, kpkt_fraction=kfrac)
    never = run(engine_mod, monkeypatch, model, cs, ts, pk0, NEVER)
    always = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALWAYS)
    assert not ran_late(engine_mod, never) and ran_late(engine_mod, always)
    print(f"{data}: kernels of the ALWAYS run {always['kinds']}; free-bound events {fb_events(always)}; k_slow launches without k_late "
          f"{never['kinds']['k_slow']['launches']}")
    same(always, never, f"k_late with the slow role vs split kernels ({data})")
    assert always["kinds"]["k_slow"]["launches"] == 0 and always["kinds"]["k_tail"]["launches"] == 0, always["kinds"]
    assert fb_events(always) > 0
    if with_oracle:
        pa, ea = pk0.copy(), abi.estimators_for(model, "classic")
        oracle.update_packets(model, cs, ts, pa, ea)
        parity.compare_packets(always["p"], pa, FLOAT_RTOL, "k_late with the slow role vs oracle")


@pytest.mark.parametrize("gridtype,ncoord", [(abi.GRID_CARTESIAN3D, 8), (abi.GRID_SPHERICAL1D, 16)])
def test_every_kind_still_comes_back(engine_mod, monkeypatch, gridtype, ncoord):
    """30 000 packets of every type: blackbody and gamma-ray kinds still leave k_late for their kernels and what they make comes back to it"""
    model, cs, ts, aux = synth.build("small", ncoord=ncoord, gridtype=gridtype)
    pk0 = synth.make_packets(model, aux, 30000, kpkt_fraction=0.2, gamma_fraction=0.1, pellet_fraction=0.1)
    never = run(engine_mod, monkeypatch, model, cs, ts, pk0, NEVER)
    always = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALWAYS)
    assert not ran_late(engine_mod, never) and ran_late(engine_mod, always)
    print(f"kernels of the ALWAYS run {always['kinds']}")
    same(always, never, "k_late with the slow role vs split kernels, every packet type")
    kinds = always["kinds"]
    assert kinds["k_gamma"]["launches"] > 0 and kinds["k_blackbody"]["launches"] > 0, kinds
    assert kinds["k_late"]["launches"] > 1, kinds  # (what the other kernels made came back)
    assert kinds["k_slow"]["launches"] == 0 and kinds["k_tail"]["launches"] == 0, kinds


@pytest.mark.parametrize("npk", [100, 257 * 64 + 1])
def test_slow_queue_partition_edges(engine_mod, monkeypatch, npk):
    """fewer packets than workgroups (a workgroup's only packet sits in the slow queue while all its other waves idle: it must be served and the
    launch must end, with no wave giving up), and one packet more than a whole number of waves"""
    model, cs, ts, aux = synth.build("small", ncoord=8)
    pk0 = synth.make_packets(model, aux, npk, kpkt_fraction=0.2, gamma_fraction=0.1, pellet_fraction=0.1)
    never = run(engine_mod, monkeypatch, model, cs, ts, pk0, NEVER)
    always = run(engine_mod, monkeypatch, model, cs, ts, pk0, ALWAYS)  # (STRICT: a bail-out would have failed the call)
    assert not ran_late(engine_mod, never) and ran_late(engine_mod, always)
    same(always, never, f"k_late with the slow role vs split kernels, {npk} packets")
    assert always["kinds"]["k_slow"]["launches"] == 0 and always["kinds"]["k_tail"]["launches"] == 0, always["kinds"]
