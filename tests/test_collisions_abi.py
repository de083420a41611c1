"""The collision bookkeeping's corner of the C ABI (mgx_collisions_*): declared in include/mgx.h, exported by both libraries,
mirrored by ctypes with the record's size, and argument validation that needs no device."""
import ctypes
import os
import re

import pytest

from magics_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mgx_collisions_enable", "mgx_collisions_update", "mgx_collisions_read", "mgx_collisions_clear")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgx.h")).read(), flags=re.S)


def test_the_four_calls_are_declared_and_bound():
    declared = set(re.findall(r"\b(mgx_[a-z0-9_]+)\s*\(", _header()))
    for name in NAMES:
        assert name in declared, name
        assert name in hostlib.SYMBOLS, name


@pytest.mark.parametrize("path", [hostlib.LIB_PATH, hostlib.FMA_LIB_PATH], ids=["libmgx", "libmgx_fma"])
def test_both_libraries_export_them(path):
    L = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(L, name), (path, name)


def test_the_event_record_is_32_bytes_in_header_and_mirror():
    assert ctypes.sizeof(hostlib.CollisionEvent) == 32
    assert hostlib.collision_event_dtype().itemsize == 32
    body = re.search(r"typedef struct mgx_collision_event \{(.*?)\} mgx_collision_event;", _header(), flags=re.S).group(1)
    fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert fields == ["uint64_t pass", "int32_t robot_a, robot_b", "float mins[2], maxs[2]"]
    dt = hostlib.collision_event_dtype()
    assert [dt.fields[n][1] for n in ("pass", "robot_a", "robot_b", "mins", "maxs")] == [0, 8, 12, 16, 24]
    assert [getattr(hostlib.CollisionEvent, n).offset for n in ("pass_", "robot_a", "robot_b", "mins", "maxs")] == [0, 8, 12, 16, 24]


def test_a_null_world_is_an_invalid_argument_without_a_device():
    L = hostlib.lib()
    n = ctypes.c_uint64()
    assert L.mgx_collisions_enable(None, 1, 0, 0) == -1
    assert L.mgx_collisions_update(None, None) == -1
    assert L.mgx_collisions_read(None, 0, None, 0, ctypes.byref(n), ctypes.byref(n), None) == -1
    assert L.mgx_collisions_clear(None) == -1
    assert b"null" in L.mgx_last_error()
