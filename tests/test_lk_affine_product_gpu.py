"""GPU: affine refinement through polychase_core (OpticalFlowOptions.affine_refinement).  The clip is tests/lk_affine_scene.py's:
6 frames of 96 x 80 (R = G = B, so gray is the channel) that roll by 1.5 degrees per frame, window 10, max_level 2; the detector
keeps its 12 strongest corners per frame.  The rows of the default run ARE the forward records with status 1, so the database of a
run with the option must hold, pair by pair, what the numpy restatement of the rule (tests/lk_affine_ref.py) makes of them."""
import functools
import os
import sqlite3
import sys

import numpy as np
import pytest

import lk_affine_ref as ref
import lk_affine_scene as scene
import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = scene.W, scene.H, 6
WIN, MAX_LEVEL = 10, 2
MAX_CORNERS = 12


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@functools.lru_cache(maxsize=None)
def _clip():
    return scene.rolling_clip(N, 1.5)


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _run(core, path, affine=None, normalize=None):
    frames = _clip()
    vi = core.VideoInfo(W, H, 1, N)
    go = core.GFTTOptions()
    go.max_corners = MAX_CORNERS
    fo = core.OpticalFlowOptions()
    fo.window_size, fo.max_level = WIN, MAX_LEVEL
    if affine is not None:
        fo.affine_refinement = affine
    if normalize is not None:
        fo.normalize = normalize
    core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, path, go, fo)
    return _dump(path)


def test_database_holds_what_the_rule_makes_of_the_default_runs_rows(core, tmp_path):
    default = _run(core, str(tmp_path / "default.db"))
    got = _run(core, str(tmp_path / "affine.db"), True)
    assert got[0] == default[0], "keypoints"
    assert sorted(got[1]) == sorted(default[1]) and len(got[1]) == sum(1 for a in range(1, N + 1) for s in (-8, -4, -2, -1, 1, 2, 4, 8) if 1 <= a + s <= N)
    with oracle.emulation(oracle.EMU_CANONICAL):
        planes = {i + 1: ref.Planes(oracle.Pyramid(np.ascontiguousarray(f[:, :, 0]), WIN, MAX_LEVEL)) for i, f in enumerate(_clip())}
    oopt = oracle.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    want, moved, total = {}, 0, 0
    for (a, b) in sorted(default[1]):
        kps = np.frombuffer(default[0][a][1], np.float32).reshape(-1, 2)
        rows, idx, xy, err = default[1][(a, b)]
        idx = np.frombuffer(idx, np.uint32)
        assert 6 <= len(kps) <= MAX_CORNERS
        q, st, e = np.zeros((len(kps), 2), np.float32), np.zeros(len(kps), np.uint8), np.zeros(len(kps), np.float32)
        q[idx], st[idx], e[idx] = np.frombuffer(xy, np.float32).reshape(-1, 2), 1, np.frombuffer(err, np.float32)
        r = ref.refine(planes[a], [planes[b]], kps, [(q, st, e)], oopt)[0]
        want[(a, b)] = (rows, idx.tobytes(), r[0][idx].tobytes(), r[2][idx].tobytes())
        total += len(idx)
        moved += int((r[4] == ref.ACCEPTED).sum()) if want[(a, b)] != default[1][(a, b)] else 0
    # asserted on the REFERENCE's result, before anything is compared with it: rows exist, and the option moves them
    print("reference rows", total, "accepted rows in pairs that changed", moved)
    assert total >= 3 * len(want) and moved >= total // 4
    for pair in sorted(want):
        assert got[1][pair] == want[pair], pair


def test_false_gives_the_file_of_a_run_that_never_sets_the_attribute(core, tmp_path, monkeypatch):
    # one transaction per frame, so that whole files can be compared (tests/test_lk_fb_gpu.py explains)
    monkeypatch.setenv("POLYCHASE_DB_BATCH_FRAMES", "1")
    a, b, c = (str(tmp_path / n) for n in ("untouched.db", "off.db", "on.db"))
    _run(core, a)
    _run(core, b, False)
    assert open(a, "rb").read() == open(b, "rb").read()
    _run(core, c, True)
    assert open(c, "rb").read() != open(a, "rb").read() and _dump(c) != _dump(a)
    _run(core, b + "2", False)      # the parked engine of the run above carries nothing over
    assert open(b + "2", "rb").read() == open(a, "rb").read()


def test_the_option_together_with_normalize_is_a_value_error(core, tmp_path):
    with pytest.raises(ValueError, match="affine_refinement"):
        _run(core, str(tmp_path / "both.db"), True, True)
    assert not os.path.exists(str(tmp_path / "both.db"))
