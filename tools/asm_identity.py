#!/usr/bin/env python3
"""Did a move-only change leave the compiler the same program?

    tools/asm_identity.py PARENT_TREE THIS_TREE [preset ...]     (default: every preset of artis_amd/build.py)

PARENT_TREE is a checkout of the parent commit (git archive <parent> | tar -x -C <scratch dir>), THIS_TREE the changed tree. For each
preset, in both trees: the device and the host assembly of artis_amd/csrc/artis_engine.hip (the flags of artis_amd.build without -shared
and -ldl, the preset's defines, -cuid=fixed -S, --cuda-device-only / --cuda-host-only) and the x86 assembly of tests/hostemu/emu.cc (g++ -S
with the CXXFLAGS of tests/hostemu/Makefile). The outputs are compared byte for byte: one line per (preset, half), `identical` or the first
line that differs; exit status 1 on any difference. A plain diff: nothing inside the assembly is looked at. FLAGS and PRESETS of the two
trees' build.py must be equal (else it stops); the preset's defines are formed by THIS_TREE's preset_flags().
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HALVES = ("device", "host", "hostemu")


def load_build(tree):
    """artis_amd/build.py of a tree, by path: nothing else of the package is imported"""
    spec = importlib.util.spec_from_file_location(f"build_{abs(hash(tree))}", os.path.join(tree, "artis_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


def commands(this_tree, build, preset):
    """half -> (directory below a tree to run in, argv without the output file)"""
    hipcc = [a for a in build.FLAGS if a not in ("-shared", "-ldl")] + build.preset_flags(preset) + ["-cuid=fixed", "-S"]
    mk = open(os.path.join(this_tree, "tests", "hostemu", "Makefile")).read()
    cxxflags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).split()
    define = [] if preset == "classic" else [f"-DARTIS_PRESET_{preset.upper()}"]
    csrc, emu = os.path.join("artis_amd", "csrc"), os.path.join("tests", "hostemu")
    return {"device": (csrc, ["hipcc", *hipcc, "--cuda-device-only", "artis_engine.hip"]),
            "host": (csrc, ["hipcc", *hipcc, "--cuda-host-only", "artis_engine.hip"]),
            "hostemu": (emu, ["g++", *cxxflags, *define, "-S", "emu.cc"])}


def first_difference(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        for n, (la, lb) in enumerate(zip(fa, fb), 1):
            if la != lb:
                return f"line {n}: {la[:120]!r} | {lb[:120]!r}"
    return "identical" if os.path.getsize(a) == os.path.getsize(b) else "one output is a prefix of the other"


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    trees = [os.path.abspath(argv[1]), os.path.abspath(argv[2])]
    parent, build = load_build(trees[0]), load_build(trees[1])
    for name in ("FLAGS", "PRESETS"):  # a move-only change changes no flag: both trees are then built alike
        if getattr(parent, name) != getattr(build, name):
            sys.exit(f"artis_amd/build.py {name} differ between the trees: {getattr(parent, name)} | {getattr(build, name)}")
    presets = argv[3:] or list(build.PRESETS)
    with tempfile.TemporaryDirectory() as out:
        jobs = []
        for preset in presets:
            for half, (sub, cmd) in commands(trees[1], build, preset).items():
                for t, tree in enumerate(trees):
                    jobs.append((os.path.join(tree, sub), [*cmd, "-o", os.path.join(out, f"{t}.{preset}.{half}.s")]))
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:  # one compiler process per worker
            list(pool.map(lambda j: subprocess.check_call(j[1], cwd=j[0]), jobs))
        bad = 0
        for preset in presets:
            for half in HALVES:
                verdict = first_difference(*(os.path.join(out, f"{t}.{preset}.{half}.s") for t in (0, 1)))
                bad += verdict != "identical"
                print(f"{preset} {half}: {verdict}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
