"""GPU: brightness-normalised LK through polychase_core (OpticalFlowOptions.normalize).  The database of a run with the option
holds the default run's keypoints, and every pair's rows are those the numpy restatement of the rule (tests/lk_normalized_ref.py)
computes from them.  The clip is that of tests/test_lk_correlation_product_gpu.py: tests/fb_scene.py's (R = G = B, so gray is
the channel), 12 frames, every second frame x 0.7 + 30, window 10, max_level 2.  The detector keeps its 12 strongest corners per
frame, so that the reference tracks about 750 (keypoint, target) pairs for the whole database."""
import functools
import os
import sqlite3
import sys

import numpy as np
import pytest

import fb_scene
import lk_correlation_ref as corr_ref
import lk_correlation_scene as scene
import lk_normalized_ref as ref
import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = scene.W, scene.H, 12
WIN, MAX_LEVEL = 10, 2
MAX_CORNERS = 12
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


def _options(core, normalize=None, min_correlation=None):
    fo = core.OpticalFlowOptions()
    fo.window_size, fo.max_level = WIN, MAX_LEVEL
    if normalize is not None:
        fo.normalize = normalize
    if min_correlation is not None:
        fo.min_correlation = min_correlation
    return fo


def _run(core, path, normalize=None, min_correlation=None, shard=None):
    frames = _clip()
    vi = core.VideoInfo(W, H, 1, N)
    go = core.GFTTOptions()
    go.max_corners = MAX_CORNERS
    fo = _options(core, normalize, min_correlation)
    if shard is None:
        core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, path, go, fo)
    else:
        core.generate_optical_flow_shard(vi, lambda fid: frames[fid - 1], None, path, shard[0], shard[1], detector_options=go, flow_options=fo)
    return _dump(path)


@pytest.fixture(scope="module")
def runs(core, tmp_path_factory):
    """the default database and the normalised one, each computed once"""
    d = tmp_path_factory.mktemp("lk_normalized")
    return _run(core, str(d / "default.db")), _run(core, str(d / "normalized.db"), True)


def _rows(flow):
    rows, idx, xy, err = flow
    return np.frombuffer(idx, np.uint32), np.frombuffer(xy, np.float32).reshape(-1, 2), np.frombuffer(err, np.float32)


def test_database_holds_the_rows_the_reference_computes_from_the_default_keypoints(runs):
    default, got = runs
    assert got[0] == default[0], "keypoints"
    assert sorted(got[1]) == sorted(default[1]) and len(got[1]) == sum(1 for a in range(1, N + 1) for s in (-8, -4, -2, -1, 1, 2, 4, 8) if 1 <= a + s <= N)
    planes = {i + 1: ref.Planes(oracle.Pyramid(np.ascontiguousarray(f[:, :, 0]), WIN, MAX_LEVEL)) for i, f in enumerate(_clip())}
    oopt = oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    want, changed, total = {}, 0, 0
    for (a, b) in sorted(default[1]):
        kps = np.frombuffer(default[0][a][1], np.float32).reshape(-1, 2)
        assert 6 <= len(kps) <= MAX_CORNERS
        xy, st, err = ref.track(planes[a], planes[b], kps, oopt)
        sel = np.nonzero(st == 1)[0]
        want[(a, b)] = (len(sel), sel.astype(np.uint32).tobytes(), xy[sel].tobytes(), err[sel].tobytes())
        total += len(sel)
        changed += want[(a, b)] != default[1][(a, b)]
    # asserted on the REFERENCE's result, before anything is compared with it: rows exist, and the option moves them
    print("reference rows", total, "pairs whose rows differ from the default run's", changed, "of", len(want))
    assert total >= 3 * len(want) and changed >= len(want) // 2
    for pair in sorted(want):
        assert got[1][pair] == want[pair], pair


def test_two_shards_give_the_one_shard_database_and_the_parked_engine_carries_nothing_over(core, runs, tmp_path):
    default, got = runs
    k1, f1 = _run(core, str(tmp_path / "s1.db"), True, shard=(1, 7))
    k2, f2 = _run(core, str(tmp_path / "s2.db"), True, shard=(7, N + 1))
    assert sorted(k1) == list(range(1, 7)) and not set(k1) & set(k2)
    assert ({**k1, **k2}, {**f1, **f2}) == got
    # the parked engine of the runs above serves this one
    assert _run(core, str(tmp_path / "default2.db")) == default


def test_false_gives_the_file_of_a_run_that_never_sets_the_attribute(core, tmp_path, monkeypatch):
    # one transaction per frame, so that whole files can be compared (tests/test_lk_fb_gpu.py explains)
    monkeypatch.setenv("POLYCHASE_DB_BATCH_FRAMES", "1")
    a, b, c = (str(tmp_path / n) for n in ("untouched.db", "off.db", "on.db"))
    _run(core, a)
    _run(core, b, False)
    assert open(a, "rb").read() == open(b, "rb").read()
    _run(core, c, True)
    assert open(c, "rb").read() != open(a, "rb").read() and _dump(c) != _dump(a)
    _run(core, b + "2", False)
    assert open(b + "2", "rb").read() == open(a, "rb").read()


def test_with_a_minimum_correlation_the_normalised_rows_are_filtered_by_that_rule(core, runs, tmp_path):
    _, normalized = runs
    keypoints, flows = normalized
    gray = {i + 1: np.ascontiguousarray(f[:, :, 0]) for i, f in enumerate(_clip())}
    want, rows, kept = {}, 0, 0
    for (a, b), flow in flows.items():
        kps = np.frombuffer(keypoints[a][1], np.float32).reshape(-1, 2)
        idx, xy, err = _rows(flow)
        q, st = np.zeros((len(kps), 2), np.float32), np.zeros(len(kps), np.uint8)
        q[idx], st[idx] = xy, 1
        k, _ = corr_ref.rows(gray[a], gray[b], WIN, kps, q, st, THR)
        sel = k[idx] == 1
        want[(a, b)] = (int(sel.sum()), idx[sel].tobytes(), xy[sel].tobytes(), err[sel].tobytes())
        rows, kept = rows + len(idx), kept + int(sel.sum())
    print("normalised rows", rows, "kept at", THR, ":", kept)
    assert 0 < kept < rows, "the filter must drop some rows and keep some (asserted on the reference)"
    got = _run(core, str(tmp_path / "both.db"), True, THR)
    assert got[0] == keypoints
    assert got[1] == want
