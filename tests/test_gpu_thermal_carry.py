"""GPU tests of k_thermal's leave rule (DESIGN.md section 3 "Hand-over at list exhaustion"): in a launch with the hand-over a packet keeps its lane
while the list lasts -- no unit budget (ARTIS_AMD_BUDGET_T_BULK, 0 = none, the default) -- and leaves for budget reasons only once the list is used
up. Where a packet is handed from launch to launch is placement: every field of every packet, generator state included, must equal the default
engine's bit for bit.

Model and packets are those of test_gpu_parity.test_budget_independence_on_device, at 20 000 packets (the kernel form with the tables in LDS in the
large launches) and at 3 000 (the plain form throughout, many short launches). The carried-first lists this file was planned for lost on the
headline and are not in the engine (profiles/r11/thermal_bulk_budget.md); runs (a) to (c) are the issue's without them."""
import numpy as np
import pytest

import parity
from artis_amd import abi, synth

pytestmark = pytest.mark.gpu

VARIABLES = ("ARTIS_AMD_DRAIN_T", "ARTIS_AMD_DRAIN_MIN", "ARTIS_AMD_BUDGET_T", "ARTIS_AMD_BUDGET_T_BULK", "ARTIS_AMD_BUDGET")
HANDOVER = {"ARTIS_AMD_DRAIN_T": "1", "ARTIS_AMD_DRAIN_MIN": "0"}  # the hand-over in every launch
RUNS = {
    "(a) hand-over in every launch, no bulk budget": HANDOVER,
    "(b) ... and a launch budget of 8 units": {**HANDOVER, "ARTIS_AMD_BUDGET_T": "8"},
    "(c) the rule of before: the launch's budget while the list lasts": {**HANDOVER, "ARTIS_AMD_BUDGET_T": "8", "ARTIS_AMD_BUDGET_T_BULK": "8"},
}


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from artis_amd import engine

    engine.load_library()
    return engine


def run(engine_mod, monkeypatch, model, cs, ts, pk0, env):
    for v in VARIABLES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_mod.Engine(model)
    eng.set_cellstate(cs, ts)
    p = pk0.copy()
    eng.update_packets(p, abi.Estimators(model["npts_nonempty"], model["nbfcontinua_ground"]))
    launches = eng.last_kernel_ms_by_kind()["k_thermal"]["launches"]
    eng.close()
    return p, launches


@pytest.mark.parametrize("npackets", [20000, 3000])
def test_leave_rule_is_placement(engine_mod, monkeypatch, npackets):
    model, cs, ts, aux = synth.build("tiny", ncoord=6)
    pk0 = synth.make_packets(model, aux, npackets, kpkt_fraction=0.3)
    ref, _ = run(engine_mod, monkeypatch, model, cs, ts, pk0, {})
    launches = {}
    for what, env in RUNS.items():
        p, launches[what] = run(engine_mod, monkeypatch, model, cs, ts, pk0, env)
        print(f"{npackets} packets {what}: {launches[what]} k_thermal launches")
        parity.compare_packets(p, ref, 0.0, what)
        assert np.array_equal(p["rngstate"], ref["rngstate"]), what
    a, b, c = (launches[w] for w in RUNS)
    # the switch is read: with 8 units per launch while the list lasts, every walk of more than 8 units comes back to the next launch; without a bulk
    # budget only what a drained launch hands over does. The short lists of 3 000 packets need many launches either way, and more under (c).
    if npackets == 3000:
        assert c > b, launches
