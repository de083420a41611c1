"""The device trackers' interface as far as it can be checked without a device: the header declares what the bindings bind, the
record is 40 bytes in every language, and Simulation refuses device trackers without device missions."""
import ctypes
import os
import re

import numpy as np
import pytest

from magics_amd import hostlib, sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["mgx_tracks_enable", "mgx_tracks_set_clock", "mgx_tracks_update", "mgx_tracks_take", "mgx_tracks_clear"]


def test_header_bindings_and_record_agree():
    header = open(os.path.join(ROOT, "include", "mgx.h"), encoding="utf-8").read()
    rust = open(os.path.join(ROOT, "rust", "magics-hip", "src", "sys.rs"), encoding="utf-8").read()
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in hostlib.SYMBOLS and "pub fn " + name + "(" in rust, name
    m = re.search(r"typedef struct mgx_track_sample \{(.*?)\} mgx_track_sample;", header, flags=re.S)
    assert m and [f for f in re.findall(r"\b(tick|robot|span_ticks|position|velocity)\b", re.sub(r"/\*.*?\*/", "", m.group(1)))] == \
        ["tick", "robot", "span_ticks", "position", "velocity"]
    dt = hostlib.track_sample_dtype()
    assert ctypes.sizeof(hostlib.TrackSample) == dt.itemsize == 40
    assert [dt.fields[f][1] for f in ("tick", "robot", "span_ticks", "position", "velocity")] == [0, 8, 12, 16, 28]
    assert [getattr(hostlib.TrackSample, f).offset for f in ("tick", "robot", "span_ticks", "position", "velocity")] == [0, 8, 12, 16, 28]
    assert "pub struct mgx_track_sample" in rust
    assert len(hostlib.SYMBOLS["mgx_tracks_enable"][1]) == 6 and len(hostlib.SYMBOLS["mgx_tracks_take"][1]) == 7


def test_device_trackers_need_device_missions():
    class NoWorld:
        pass
    with pytest.raises(ValueError, match="device_trackers needs device_missions"):
        sim.Simulation({"config": {}, "environment": {}, "formation": {"formations": []}}, NoWorld(), device_missions=False, device_trackers=True)


def test_sample_dtype_views_a_record():
    rec = hostlib.TrackSample(7, 3, 2, (ctypes.c_float * 3)(1.0, -1.5, 2.0), (ctypes.c_float * 3)(0.5, 0.0, -0.25))
    a = np.frombuffer(bytes(rec), dtype=hostlib.track_sample_dtype())
    assert (int(a["tick"][0]), int(a["robot"][0]), int(a["span_ticks"][0])) == (7, 3, 2)
    assert a["position"][0].tolist() == [1.0, -1.5, 2.0] and a["velocity"][0].tolist() == [0.5, 0.0, -0.25]
