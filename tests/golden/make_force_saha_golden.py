"""Regenerate tests/golden/force_saha_reference.json from the REFERENCE's own options files.

    python tests/golden/make_force_saha_golden.py <reference source tree>

Needs the reference's source tree. For every artisoptions_*.h found there, a two-line harness (written to a temporary directory, nothing
of the reference is copied) includes the file and prints FORCE_SAHA_ION_BALANCE(Z) for Z = 1..100. Stores, per options file, whether
it is the same for every Z and its value. tests/test_ion_balance_rules.py pins ARTIS_OPT_FORCE_SAHA_ION_BALANCE of every preset of
include/artis_options.h that stands for one of these files against it.
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
int main() { for (int z = 1; z <= 100; z++) std::printf("%d\\n", static_cast<int>(FORCE_SAHA_ION_BALANCE(z))); }
"""


def main():
    reference = sys.argv[1]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "force_saha.cc")
        with open(src, "w") as f:
            f.write(HARNESS)
        for path in sorted(glob.glob(os.path.join(reference, "artisoptions_*.h"))):
            name = os.path.basename(path)[len("artisoptions_"):-2]
            exe = os.path.join(tmp, name)
            subprocess.check_call(["g++", "-std=c++20", "-I", reference, f'-DOPTFILE="{os.path.basename(path)}"', "-o", exe, src])
            vals = [int(x) for x in subprocess.check_output([exe]).split()]
            out[name] = {"constant": len(set(vals)) == 1, "value": bool(vals[0])}
    with open(os.path.join(HERE, "force_saha_reference.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
