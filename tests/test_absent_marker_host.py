"""The "not populated" marker of a macro-atom record (absent ions), on the CPU: tests/mamarker_host/marker_main.cc compiles
physics.h for x86 and checks that the marker passes the transition loop's `unusable` test, differs from populate_mafilter_level()'s own "no
usable filter" marker, and is written by populate_mafilter_level() for no rates -- random ones over 86 decades, a zero total, a negative rate, a
rate that is not finite; and that rng_unstep() puts the generator back where it stood before a draw."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_marker_is_unusable_distinct_and_never_a_filter(tmp_path):
    exe = str(tmp_path / "marker_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(HERE, "mamarker_host", "marker_main.cc")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    last = res.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 failed") and not last.startswith("0 cases"), last
