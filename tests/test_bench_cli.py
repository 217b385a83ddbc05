"""bench.py's command line: a plain run does what the headline figure needs and nothing else; --full adds the measurements that take
runs of their own (the CPU baseline). The GPU test runs main() on a small workload with the CPU leg replaced by a recorder, so that it
checks the wiring and not the oracle's speed."""
import json

import pytest

import bench

SMALL = ["--preset", "small", "--ncoord", "8", "--packets", "5000", "--steps", "1", "--warmup", "1"]
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_full_is_off_by_default_and_gates_the_cpu_baseline():
    plain = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert plain.full is False and (plain.steps, plain.warmup) == (3, 2)
    assert not bench.cpu_baseline_wanted(plain, 0, 1)
    assert not bench.cpu_baseline_wanted(bench.parse_args(["--no-cpu-baseline"]), 0, 1)  # (the option of the existing scripts still parses)
    full = bench.parse_args(["--full"])
    assert full.full is True and bench.cpu_baseline_wanted(full, 0, 1)
    assert not bench.cpu_baseline_wanted(full, 1, 1) and not bench.cpu_baseline_wanted(full, 0, 2)  # rank 0 of a single-GPU run only
    assert not bench.cpu_baseline_wanted(bench.parse_args(["--full", "--no-cpu-baseline"]), 0, 1)
    assert not bench.cpu_baseline_wanted(bench.parse_args(["--full", "--cpu-sample", "0"]), 0, 1)
    assert bench.cpu_baseline_wanted(bench.parse_args(["--full", "--cpu-both"]), 0, 1)


def test_cpu_both_without_full_is_an_error():
    with pytest.raises(SystemExit) as exc:
        bench.parse_args(["--cpu-both"])
    assert exc.value.code == 2


@pytest.mark.gpu
def test_plain_run_skips_what_full_measures(monkeypatch, capsys):
    calls = []

    def recorder(model, cs, ts, pk, sample, cores, options="classic", both=False):
        calls.append((sample, both))
        return {"value": 1000.0, "unit": "packet-steps/s", "cores": cores, "kind": "recorder"}

    monkeypatch.setattr(bench, "cpu_baseline", recorder)
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--cpu-sample", "700"])):
        bench.main(SMALL + extra)
        printed = capsys.readouterr().out.strip().splitlines()
        assert len(printed) == 1, printed  # ONE result line
        lines[name] = json.loads(printed[0])
        assert calls == ([] if name == "plain" else [(700, False)])
    plain, full = lines["plain"], lines["full"]
    assert "cpu_baseline" not in plain and "gpu_over_cpu_baseline" not in plain
    assert full["cpu_baseline"]["kind"] == "recorder" and full["gpu_over_cpu_baseline"] == full["value"] / 1000.0
    for line in (plain, full):
        assert all(k in line for k in HEADLINE_KEYS)
        assert (line["metric"], line["unit"], line["higher_is_better"], line["dtype"]) == ("packet-steps/sec", "packet-steps/s", True, "f64")
        assert line["value"] > 0 and line["ms_per_step"] > 0
    # the same seeded workload in both runs: --full changes what is measured beside the steps, not the steps
    assert plain["config"]["packet_steps_per_step"] == full["config"]["packet_steps_per_step"] > 0
    assert set(full) - set(plain) == {"cpu_baseline", "gpu_over_cpu_baseline"}
