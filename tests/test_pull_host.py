"""The work-pulling rules of the propagation kernels (artis_amd/csrc/work_pull.h: Puller, chunk_at, pull_wave) compiled for x86 under
ARTIS_HOST_EMU and driven by tests/pull_host/pull_main.cc: simulated waves pull from lists of 0 ... 50 000 entries cut into 8 ... 8192 chunks, and
every index must be handed out exactly once."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_index_is_handed_out_exactly_once(tmp_path):
    exe = str(tmp_path / "pull_main")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "pull_host", "pull_main.cc")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    last = res.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 failed") and not last.startswith("0 cases"), last
