"""GPU: masked LK windows through polychase_core (OpticalFlowOptions.mask_windows with detection_mask=).  Every pair's rows in the
database must be the stage-level rows of pc_lk_track_window_masked -- which tests/test_lk_window_mask_gpu.py pins to the numpy
restatement of the rule -- for the keypoints the database holds; the clip is tests/lk_window_mask_scene.py's two-layer scene, the
mask a polygon that follows its disc from frame to frame."""
import functools
import os
import sqlite3
import sys
import time

import numpy as np
import pytest

import lk_window_mask_scene as scene
from polychase_amd import hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 160, 120, 12
WIN, MAX_LEVEL = 10, 2
SKIPS = (-8, -4, -2, -1, 1, 2, 4, 8)


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


def _time(fid):
    return (fid - 1) / 3.0


@functools.lru_cache(maxsize=None)
def _clip():
    return [np.ascontiguousarray(np.repeat(scene.frame(_time(f))[0][:H, :W, None], 3, axis=2)) for f in range(1, N + 1)]


def _outline(fid):
    """the disc of frame fid as a 48-gon"""
    a = 2.0 * np.pi * np.arange(48) / 48
    cx, cy = scene.CENTRE[0] + _time(fid) * scene.FG_MOTION[0], scene.CENTRE[1] + _time(fid) * scene.FG_MOTION[1]
    return np.stack([cx + scene.RADIUS * np.cos(a), cy + scene.RADIUS * np.sin(a)], axis=1).astype(np.float32)


def _masks(core):
    return {fid: core.PolygonMask([_outline(fid)]) for fid in range(1, N + 1)}


def _options(core, **kw):
    fo = core.OpticalFlowOptions()
    fo.window_size, fo.max_level = WIN, MAX_LEVEL
    for k, v in kw.items():
        setattr(fo, k, v)
    return fo


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _run(core, path, mask, fo):
    frames = _clip()
    core.generate_optical_flow_database(core.VideoInfo(W, H, 1, N), lambda fid: frames[fid - 1], None, path, core.GFTTOptions(), fo,
                                        detection_mask=mask)
    return _dump(path)


def _stage_rows(kps, mask_windows, fb):
    """what the database must hold, from the stage-level call on the database's keypoints -> flows, touched keypoints, rows"""
    ctx = hip.Context(0)
    fr = {}
    for fid in range(1, N + 1):
        f = hip.Frame(ctx, W, H, WIN, MAX_LEVEL)
        f.set_rgb(_clip()[fid - 1])
        f.set_mask_polygons([_outline(fid)])
        fr[fid] = f
    opt = hip.flow_options(window_size=WIN, max_level=MAX_LEVEL)
    want, touched = {}, 0
    for a in range(1, N + 1):
        tg = [a + s for s in SKIPS if 1 <= a + s <= N]
        n, blob = kps[a]
        fr[a].set_keypoints(np.frombuffer(blob, np.float32).reshape(n, 2))
        xy, st, err, _, _, tch = hip.lk_track_window_masked(ctx, fr[a], [fr[b] for b in tg], mask_windows, fb, -1, opt)
        touched += int(tch.sum())
        for k, b in enumerate(tg):
            keep = np.nonzero(st[k] == 1)[0].astype(np.uint32)
            want[(a, b)] = (len(keep), keep.tobytes(), xy[k][keep].tobytes(), err[k][keep].tobytes())
    for f in fr.values():
        f.close()
    ctx.close()
    return want, touched


@pytest.mark.parametrize("fb", [0.0, 1.0])
def test_database_rows_are_the_stage_level_rows(core, tmp_path, fb):
    got = _run(core, str(tmp_path / "on.db"), _masks(core), _options(core, mask_windows=True, forward_backward_threshold=fb))
    assert sorted(got[0]) == list(range(1, N + 1)) and min(v[0] for v in got[0].values()) >= 10
    want, touched = _stage_rows(got[0], 1, fb)
    plain, _ = _stage_rows(got[0], 0, fb)
    assert touched >= N and want != plain, "keypoints detected under the disc lie near its outline, and the rule moves their rows"
    assert sorted(got[1]) == sorted(want)
    for key in sorted(want):
        assert got[1][key] == want[key], key
    assert sum(v[0] for v in want.values()) >= 20 * len(want)


def test_option_off_is_byte_identical_to_a_run_that_never_names_the_field(core, tmp_path, monkeypatch):
    # one transaction per frame, so that whole files can be compared (tests/test_lk_fb_gpu.py explains)
    monkeypatch.setenv("POLYCHASE_DB_BATCH_FRAMES", "1")
    a, b, c, d = (str(tmp_path / n) for n in ("unnamed.db", "off.db", "on.db", "on_no_mask.db"))
    _run(core, a, _masks(core), _options(core))
    _run(core, b, _masks(core), _options(core, mask_windows=False))
    assert open(a, "rb").read() == open(b, "rb").read()
    _run(core, c, _masks(core), _options(core, mask_windows=True))
    assert _dump(c)[0] == _dump(a)[0] and _dump(c)[1] != _dump(a)[1], "the same keypoints, other rows"
    _run(core, b + "2", _masks(core), _options(core))        # the parked engine served the option: nothing is carried over
    assert open(b + "2", "rb").read() == open(a, "rb").read()
    _run(core, d, None, _options(core, mask_windows=True))   # nothing to weight by
    _run(core, d + "2", None, _options(core))
    assert open(d, "rb").read() == open(d + "2", "rb").read()


@pytest.mark.parametrize("other", [{"normalize": True}, {"affine_refinement": True}, {"search_radius": 16}, {"min_correlation": 0.5}])
def test_combinations_that_do_not_weight_their_windows_raise_value_error(core, tmp_path, other):
    asked = []

    def accessor(fid):
        asked.append(fid)
        return _clip()[fid - 1]

    with pytest.raises(ValueError, match="mask_windows"):
        core.generate_optical_flow_database(core.VideoInfo(W, H, 1, N), accessor, None, str(tmp_path / "x.db"), core.GFTTOptions(),
                                            _options(core, mask_windows=True, **other), detection_mask=_masks(core))
    assert asked == [], "refused before a frame is asked for"
    with pytest.raises(ValueError, match="mask_windows"):
        core.generate_optical_flow_shard(core.VideoInfo(W, H, 1, N), accessor, None, str(tmp_path / "y.db"), 1, 5,
                                         flow_options=_options(core, mask_windows=True, **other), detection_mask=_masks(core))


def test_optical_flow_thread_accepts_the_option(core, tmp_path):
    frames = _clip()
    path = str(tmp_path / "thread.db")
    th = core.OpticalFlowThread(core.VideoInfo(W, H, 1, N), path, core.GFTTOptions(), _options(core, mask_windows=True), detection_mask=_masks(core))
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
    assert _dump(path) == _run(core, str(tmp_path / "direct.db"), _masks(core), _options(core, mask_windows=True))
