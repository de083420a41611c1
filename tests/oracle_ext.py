"""The CPU oracle with the two run-time mutators it lacks (tests/cpu_oracle_ext/oracle_ext.c: the oracle's own source plus
orc_set_safety_multiplier and orc_set_tracking_path), built into a temporary directory with the flags of oracle/Makefile's
default target, and an OracleWorld over it with the two methods magics_amd.World has."""
import atexit
import ctypes as C
import os
import re
import shlex
import shutil
import subprocess
import tempfile

import numpy as np

from oracle.binding import OracleWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_oracle_ext", "oracle_ext.c")
_PATH = None


def makefile_flags():
    """CFLAGS of oracle/Makefile (its default target compiles `$(CC) $(CFLAGS) -shared -o $@ $< -lm`)"""
    text = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    m = re.search(r"^CFLAGS\s*\??=\s*(.*)$", text, flags=re.M)
    if m is None:
        raise RuntimeError("oracle/Makefile has no `CFLAGS ?= ...` line to take the oracle's compiler flags from")
    return shlex.split(m.group(1))


def lib_path():
    """the extended library, compiled once per process"""
    global _PATH
    if _PATH is None:
        d = tempfile.mkdtemp(prefix="oracle_ext_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        out = os.path.join(d, "libgbp_oracle_ext.so")
        subprocess.run(shlex.split(os.environ.get("CC", "gcc")) + makefile_flags() + ["-shared", "-o", out, SRC, "-lm"], check=True, capture_output=True)
        _PATH = out
    return _PATH


class ExtOracleWorld(OracleWorld):
    def __init__(self, params, threads=1):
        super().__init__(params, threads=threads, lib_path=lib_path())
        self._L.orc_set_safety_multiplier.argtypes = [C.c_void_p, C.c_double]
        self._L.orc_set_tracking_path.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32]

    def set_safety_multiplier(self, multiplier):
        self._chk(self._L.orc_set_safety_multiplier(self._w, float(multiplier)))

    def set_tracking_path(self, robot, path):
        path = np.ascontiguousarray(path, dtype=np.float32).reshape(-1, 2)
        self._chk(self._L.orc_set_tracking_path(self._w, robot, path.ctypes.data, path.shape[0]))


def make_pair(sc):
    """engine and extended oracle, populated with the same scenario"""
    from magics_amd import World, scenarios as S
    eng, ref = World(sc["params"]), ExtOracleWorld(sc["params"])
    assert S.populate(eng, sc) == S.populate(ref, sc)
    return eng, ref

