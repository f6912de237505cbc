"""The route of the obstacle tracks (csrc/pmaf_route.hpp, include/pmaf.h "obstacle tracks") without a device:
Route::carries_field_tracks is true exactly where k_rollout_w64_ftrack exists -- the one-slot wave-per-agent kernel of the
default arithmetic policy without the priority-slicing loop, the repulsive track's condition -- and Input::field_tracked
moves no field the rule decides. Drives tests/cpp/route_ftrack_table.cpp over tests/test_route.py's grid."""
import hashlib
import os
import subprocess

import numpy as np

import conftest
import test_route as tr
import test_sentinel_track as tst

ROOT = conftest.ROOT


def test_route_carries_field_tracks_exactly_on_the_one_slot_default_policy_kernel(tmp_path):
    exes = {}
    for name in ("route_table", "route_ftrack_table"):
        exes[name] = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(tst.ROCM, "include"),
                            "-I" + tst.CSRC, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exes[name]], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
    rows = tst._grid_rows()
    plain = tst._run(exes["route_table"], rows)
    assert hashlib.sha256(plain).hexdigest() == tst.UNTRACKED_GRID_SHA256
    base = np.array(plain.decode().split(), dtype=np.int64).reshape(len(rows), len(tr.OUT))
    g = {k: base[:, i] for i, k in enumerate(tr.OUT)}
    col = {k: rows[:, tr.IN.index(k)] for k in ("M", "math", "dpp", "plain")}
    want = (g["family"] == tr.WAVE_PER_AGENT) & (g["slots"] == 1) & (g["tiles"] == 1) & (col["math"] == tr.XACT) & (g["sliced"] == 0)
    # the whole grid with and without field tracks; both kinds of track on every seventh row
    for tracked, ftracked, pick in ((0, 0, slice(None)), (0, 1, slice(None)), (1, 1, slice(0, None, 7)), (1, 0, slice(3, None, 7))):
        sub = rows[pick]
        flags = np.tile(np.array([[tracked, ftracked]], dtype=np.int64), (len(sub), 1))
        out = tst._run(exes["route_ftrack_table"], np.concatenate([flags, sub], axis=1))
        o = np.array(out.decode().split(), dtype=np.int64).reshape(len(sub), len(tr.OUT) + 2)
        # tracks never move a handle to another kernel: the fields the rule decides do not depend on either input
        np.testing.assert_array_equal(o[:, :-2], base[pick])
        np.testing.assert_array_equal(o[:, -1], want[pick].astype(np.int64))
        np.testing.assert_array_equal(o[:, -2], o[:, -1])      # the same conditions as carries_track
    assert want.sum() > 1000 and (~want).sum() > 1000
    # the boundary rows: every family but the wave per agent refuses, and so do 61 obstacles (60 do not), the other
    # policies and the sliced loop; both ordered sums and both steps carry tracks
    assert not want[g["family"] != tr.WAVE_PER_AGENT].any()
    assert not want[col["M"] >= 61].any() and want[col["M"] == 60].any()
    assert not want[col["math"] != tr.XACT].any()
    assert not want[g["sliced"] == 1].any() and (g["sliced"] == 1).any()
    for k in ("dpp", "plain"):
        assert want[col[k] == 0].any() and want[col[k] == 1].any()
