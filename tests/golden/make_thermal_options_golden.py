"""Regenerate tests/golden/thermal_options_reference.json from the REFERENCE's own options files.

    python tests/golden/make_thermal_options_golden.py <reference source tree>

Needs the reference's source tree. For every artisoptions_*.h found there, a two-line harness (written to a temporary directory, nothing
of the reference is copied) includes the file and prints TEMPERATURE_SOLVER_ACCURACY with 17 digits. tests/test_thermal_balance_rules.py
pins ARTIS_OPT_TEMPERATURE_SOLVER_ACCURACY of every preset of include/artis_options.h that stands for one of these files against it.
"""
import glob
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = """#include <cstdio>
#include OPTFILE
int main() { std::printf("%.17g\\n", static_cast<double>(TEMPERATURE_SOLVER_ACCURACY)); }
"""


def main():
    reference = sys.argv[1]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "thermal_options.cc")
        with open(src, "w") as f:
            f.write(HARNESS)
        for path in sorted(glob.glob(os.path.join(reference, "artisoptions_*.h"))):
            name = os.path.basename(path)[len("artisoptions_"):-2]
            exe = os.path.join(tmp, name)
            subprocess.check_call(["g++", "-std=c++20", "-I", reference, f'-DOPTFILE="{os.path.basename(path)}"', "-o", exe, src])
            out[name] = {"TEMPERATURE_SOLVER_ACCURACY": float(subprocess.check_output([exe]).split()[0])}
    with open(os.path.join(HERE, "thermal_options_reference.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
