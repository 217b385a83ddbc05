"""The x86 harnesses of the tests (tests/hostemu, tests/*_host): made on first use, one library per options preset."""
import ctypes
import fcntl
import os
import subprocess

_LIBS = {}


def load(directory: str, libname_for_preset, preset: str, only_this: bool = False):
    """run make in `directory` (one at a time: pytest-xdist workers) and load libname_for_preset(preset) from it, once per process.
    only_this: make that library alone, not every preset's (a GPU test that needs one preset of a harness with many)"""
    key = (directory, preset)
    if key not in _LIBS:
        with open(os.path.join(directory, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-C", directory] + ([libname_for_preset(preset)] if only_this else []), stdout=subprocess.DEVNULL)
        _LIBS[key] = ctypes.CDLL(os.path.join(directory, libname_for_preset(preset)))
    return _LIBS[key]
