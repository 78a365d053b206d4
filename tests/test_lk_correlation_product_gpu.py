"""GPU: minimum correlation through polychase_core (OpticalFlowOptions.min_correlation).  The database of a run with the option
must be the database of the default run with every pair's rows filtered by the numpy restatement of the rule
(tests/lk_correlation_ref.py).  The clip is tests/fb_scene.py's (R = G = B, so gray is the channel) with every second frame
x 0.7 + 30: every pair across an odd skip sees the exposure change the patch error cannot tell from drift."""
import functools
import os
import sqlite3
import sys

import numpy as np
import pytest

import fb_scene
import lk_correlation_ref as ref
import lk_correlation_scene as scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = scene.W, scene.H, 12
WIN, MAX_LEVEL = 10, 2
THR = 0.75


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@functools.lru_cache(maxsize=None)
def _clip():
    frames = fb_scene.clip(W, H, N)
    return [f if i % 2 == 0 else np.ascontiguousarray(np.repeat(scene.gain(f[:, :, 0], 0.7, 30.0)[:, :, None], 3, axis=2))
            for i, f in enumerate(frames)]


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _options(core, value=None):
    fo = core.OpticalFlowOptions()
    fo.window_size, fo.max_level = WIN, MAX_LEVEL
    if value is not None:
        fo.min_correlation = value
    return fo


def _run(core, path, value=None, shard=None):
    frames = _clip()
    vi = core.VideoInfo(W, H, 1, N)
    if shard is None:
        core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, path, core.GFTTOptions(), _options(core, value))
    else:
        core.generate_optical_flow_shard(vi, lambda fid: frames[fid - 1], None, path, shard[0], shard[1], flow_options=_options(core, value))
    return _dump(path)


def _filtered(default):
    """the default database with every pair's rows filtered by the reference -> (database, {pair: (rows, kept)})"""
    keypoints, flows = default
    gray = {i + 1: np.ascontiguousarray(f[:, :, 0]) for i, f in enumerate(_clip())}
    out, counts = {}, {}
    for (a, b), (rows, idx, xy, err) in flows.items():
        kps = np.frombuffer(keypoints[a][1], np.float32).reshape(-1, 2)
        idx, xy, err = np.frombuffer(idx, np.uint32), np.frombuffer(xy, np.float32).reshape(-1, 2), np.frombuffer(err, np.float32)
        assert len(idx) == rows == len(xy) == len(err)
        q, st = np.zeros((len(kps), 2), np.float32), np.zeros(len(kps), np.uint8)
        q[idx], st[idx] = xy, 1
        k, _ = ref.rows(gray[a], gray[b], WIN, kps, q, st, THR)
        sel = k[idx] == 1
        out[(a, b)] = (int(sel.sum()), idx[sel].tobytes(), xy[sel].tobytes(), err[sel].tobytes())
        counts[(a, b)] = (rows, int(sel.sum()))
    return (keypoints, out), counts


def test_database_is_the_default_database_filtered_by_the_reference(core, tmp_path):
    default = _run(core, str(tmp_path / "default.db"))
    want, counts = _filtered(default)
    # asserted on the REFERENCE's result, before anything is compared with it: some rows dropped and some kept for every pair
    assert len(counts) == sum(1 for a in range(1, N + 1) for s in (-8, -4, -2, -1, 1, 2, 4, 8) if 1 <= a + s <= N)
    for pair, (rows, kept) in sorted(counts.items()):
        assert rows >= 10 and 0 < kept < rows, (pair, rows, kept)
    print("rows", sum(r for r, _ in counts.values()), "kept", sum(k for _, k in counts.values()))
    got = _run(core, str(tmp_path / "corr.db"), THR)
    assert got[0] == want[0], "keypoints"
    assert sorted(got[1]) == sorted(want[1])
    for pair in sorted(want[1]):
        assert got[1][pair] == want[1][pair], pair
    # two shards give the one-shard database
    k1, f1 = _run(core, str(tmp_path / "s1.db"), THR, shard=(1, 7))
    k2, f2 = _run(core, str(tmp_path / "s2.db"), THR, shard=(7, N + 1))
    assert sorted(k1) == list(range(1, 7)) and not set(k1) & set(k2)
    assert ({**k1, **k2}, {**f1, **f2}) == got
    # the parked engine of the runs above serves this one: nothing is carried over
    assert _run(core, str(tmp_path / "default2.db")) == default


def test_zero_gives_the_file_of_a_run_that_never_sets_the_attribute(core, tmp_path, monkeypatch):
    # one transaction per frame, so that whole files can be compared (tests/test_lk_fb_gpu.py explains)
    monkeypatch.setenv("POLYCHASE_DB_BATCH_FRAMES", "1")
    a, b, c = (str(tmp_path / n) for n in ("untouched.db", "zero.db", "on.db"))
    _run(core, a)
    _run(core, b, 0.0)
    assert open(a, "rb").read() == open(b, "rb").read()
    _run(core, c, THR)
    assert _dump(c) != _dump(a)
    _run(core, b + "2", 0.0)
    assert open(b + "2", "rb").read() == open(a, "rb").read()
