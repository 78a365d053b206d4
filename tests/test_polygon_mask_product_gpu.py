"""GPU: polygon detection masks through polychase_core (detection_mask= PolygonMask | callable | dict, OpticalFlowThread).
Every run is compared with the same run under the byte masks that tests/polygon_mask_ref.py gives for the same polygons: the
two databases must dump identically.  The byte-mask path itself is checked against the CPU reference in
tests/test_detection_mask_gpu.py."""
import functools
import os
import sqlite3
import sys
import time

import numpy as np
import pytest

import polygon_mask_ref as ref
from polychase_amd import hip, synth
from polychase_amd.pipeline import ClipAnalyzer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 320, 200, 12


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@functools.lru_cache(maxsize=None)
def _clip():
    c = synth.NoiseClip(W, H, N)
    return [c.frame(i) for i in range(N)]


@functools.lru_cache(maxsize=None)
def _moving_plane(fid):
    """the byte mask of frame `fid`: the reference plane of its polygons, or None"""
    polys = ref.moving(fid, W, H)
    if polys is None:
        return None
    m = ref.plane(polys, W, H)
    m.setflags(write=False)
    return m


def _moving_polygons(core, fid):
    polys = ref.moving(fid, W, H)
    return None if polys is None else core.PolygonMask(polys)


def _static_polygons():
    return ref.star(W, H) + ref.rectangle(W, H)


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _run(core, path, mask, thr=None, shard=None):
    frames = _clip()
    fo = core.OpticalFlowOptions()
    if thr is not None:
        fo.forward_backward_threshold = thr
    vi = core.VideoInfo(W, H, 1, N)
    if shard is None:
        core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, path, core.GFTTOptions(), fo, detection_mask=mask)
    else:
        core.generate_optical_flow_shard(vi, lambda fid: frames[fid - 1], None, path, shard[0], shard[1], flow_options=fo,
                                         detection_mask=mask)
    return _dump(path)


@pytest.fixture(scope="module")
def byte_run(core, tmp_path_factory):
    """the run with a callable that returns the reference planes: what every polygon run must reproduce"""
    k, f = _run(core, str(tmp_path_factory.mktemp("bytes") / "bytes.db"), _moving_plane)
    assert set(k) | {9} == set(range(1, N + 1)) and k.get(9, (0, b""))[0] == 0 and min(k[a][0] for a in k if a != 9) > 0
    assert len({k[a][1] for a in k if a != 9}) == N - 1, "every frame has keypoints of its own"
    return k, f


def test_a_callable_that_returns_moving_polygons(core, byte_run, tmp_path):
    asked = []

    def mask(fid):
        asked.append(fid)
        return _moving_polygons(core, fid)

    assert _run(core, str(tmp_path / "poly.db"), mask) == byte_run
    assert asked == list(range(1, N + 1)), "asked once per detected frame, in order"


def test_the_same_masks_as_a_dict(core, byte_run, tmp_path):
    table = {fid: _moving_polygons(core, fid) for fid in range(1, N + 1)}
    assert table[4] is None
    assert _run(core, str(tmp_path / "dict.db"), table) == byte_run
    del table[4]                                      # a missing key is no mask, as None is
    table[99] = core.PolygonMask(ref.bow_tie(W, H))   # a key beyond the clip is never looked up
    assert _run(core, str(tmp_path / "dict2.db"), table) == byte_run


def test_the_same_dict_through_the_thread(core, byte_run, tmp_path):
    frames = _clip()
    table = {fid: _moving_polygons(core, fid) for fid in range(1, N + 1)}
    path = str(tmp_path / "thread.db")
    th = core.OpticalFlowThread(core.VideoInfo(W, H, 1, N), path, detection_mask=table)
    table.clear()                                     # copied at construction
    errors, done, t0 = [], False, time.time()
    while not done and time.time() - t0 < 120:
        msg = th.try_pop()
        if msg is None:
            time.sleep(0.0005)
        elif isinstance(msg, core.OpticalFlowRequest):
            th.provide_frame(msg.frame_id, frames[msg.frame_id - 1])
        elif isinstance(msg, core.CppException):
            errors.append(msg.what())
        elif msg is True:
            done = True
    th.join()
    assert done and errors == []
    assert _dump(path) == byte_run


def test_a_static_polygon_mask_is_the_static_plane(core, tmp_path):
    polys = _static_polygons()
    a = _run(core, str(tmp_path / "static_poly.db"), core.PolygonMask(polys))
    b = _run(core, str(tmp_path / "static_bytes.db"), ref.plane(polys, W, H))
    assert a == b and min(v[0] for v in a[0].values()) > 0
    # inverted
    c = _run(core, str(tmp_path / "inv_poly.db"), core.PolygonMask(polys, invert=True))
    d = _run(core, str(tmp_path / "inv_bytes.db"), ref.plane(polys, W, H, invert=True))
    assert c == d and c != a
    # the parked engine of the masked runs serves this one: it must have carried nothing over
    e = _run(core, str(tmp_path / "plain.db"), None)
    f = _run(core, str(tmp_path / "all_on.db"), core.PolygonMask([], invert=True))
    assert e == f and e != a


def test_two_shards_give_the_records_of_one(core, byte_run, tmp_path):
    mask = functools.partial(_moving_polygons, core)
    k1, f1 = _run(core, str(tmp_path / "s1.db"), mask, shard=(1, 7))
    k2, f2 = _run(core, str(tmp_path / "s2.db"), mask, shard=(7, N + 1))
    assert sorted(k1) == list(range(1, 7)) and not set(k1) & set(k2)
    assert ({**k1, **k2}, {**f1, **f2}) == byte_run


def test_a_resumed_run_keeps_the_stored_keypoints_and_never_asks(core, byte_run, tmp_path):
    path = str(tmp_path / "resume.db")
    k1, f1 = _run(core, path, functools.partial(_moving_polygons, core), shard=(1, 7))
    asked = []

    def other(fid):
        asked.append(fid)
        return core.PolygonMask(_static_polygons())

    k2, f2 = _run(core, path, other)
    assert asked == list(range(7, N + 1)), "frames whose keypoints row exists are not asked about"
    assert {a: k2[a] for a in k1} == k1 and {p: f2[p] for p in f1} == f1
    static = _run(core, str(tmp_path / "static.db"), ref.plane(_static_polygons(), W, H))[0]
    assert {a: k2[a] for a in range(7, N + 1)} == {a: static[a] for a in range(7, N + 1)}
    # a dict is looked up for the same frames only: its entries for stored frames are dead
    path2 = str(tmp_path / "resume2.db")
    _run(core, path2, functools.partial(_moving_polygons, core), shard=(1, 7))
    table = {fid: core.PolygonMask(ref.bow_tie(W, H) if fid < 7 else _static_polygons()) for fid in range(1, N + 1)}
    assert _run(core, path2, table) == (k2, f2)


def test_with_the_forward_backward_check_on_top(core, byte_run, tmp_path):
    a = _run(core, str(tmp_path / "fb_poly.db"), functools.partial(_moving_polygons, core), thr=1.0)
    b = _run(core, str(tmp_path / "fb_bytes.db"), _moving_plane, thr=1.0)
    assert a == b
    assert a[0] == byte_run[0], "the check keeps the keypoints"


def _launches(polygons):
    """launches per kernel class of 12 pipelined steps under a static mask, as in tests/test_detection_mask_device_gpu.py"""
    clip = synth.NoiseClip(W, H, 40)
    frames = [clip.frame(i) for i in range(40)]
    ctx = hip.Context(0)
    an = ClipAnalyzer(ctx, W, H, 1, 40, lambda f: frames[f - 1])
    if polygons:
        an.an.set_mask_polygons(ref.star(W, H))
    else:
        an.an.set_mask(ref.plane(ref.star(W, H), W, H))
    an.run(range(9, 13), None)
    ctx.synchronize()
    ctx.enable_timing(True)
    ctx.reset_timing()
    kept = {}
    an.run(range(13, 25), lambda frame1, kps, detected, flows: kept.__setitem__(frame1, kps.copy()))
    counts = {k: v[0] for k, v in ctx.timing().items()}
    ctx.enable_timing(False)
    an.close()
    ctx.close()
    return counts, kept


def test_polygons_enqueue_the_launches_of_a_byte_mask_in_every_existing_class():
    """the rasteriser replaces the plane's copy; nothing else changes, and it belongs to no timed class"""
    cp, kp = _launches(True)
    cb, kb = _launches(False)
    print("launches of 12 steps under polygons:", cp)
    assert cp == cb and cp["min_eig"] == 12 and cp["nms"] == 12
    assert sorted(kp) == sorted(kb) == list(range(13, 25))
    assert all(kp[a].tobytes() == kb[a].tobytes() and len(kp[a]) > 0 for a in kp)
