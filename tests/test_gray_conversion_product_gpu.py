"""GPU: the gray conversion through polychase_core (OpticalFlowOptions.channel_weights / float_transfer / float_exposure).  The clip
is tests/lk_affine_scene.py's rolling clip, 10 frames of 96 x 80, window 10, max_level 2.  Two equalities, neither a tolerance:

  * the clip linearised with the sRGB EOTF and darkened by 4 stops, handed over as float32 RGBA, under float_transfer = "srgb" and
    float_exposure = 4 gives the `keypoints` and `optical_flow` rows of the uint8 clip -- the planes are the same bytes
    (tests/test_gray_conversion_cpu.py has the round trip of the 256 codes);
  * a clip whose three channels differ, under channel_weights = (0, 0, 1), gives the rows of the clip with B in every channel;
    under weights whose quantisation needs rounding, a residual and a tie-break it gives the rows of the clip that holds the numpy
    rule's gray plane in every channel.

Both through the database call, through OpticalFlowThread and as 2 shards against 1; and with every option at its default the file
is the one of a run that never touched them."""
import functools
import os
import sqlite3
import sys
import time

import numpy as np
import pytest

import gray_conversion_ref as ref
import lk_affine_scene as scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = scene.W, scene.H, 10
WIN, MAX_LEVEL = 10, 2
PAIRS = sum(1 for a in range(1, N + 1) for s in (-8, -4, -2, -1, 1, 2, 4, 8) if 1 <= a + s <= N)


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@functools.lru_cache(maxsize=None)
def _clips():
    u8 = scene.rolling_clip(N, 0.8)                     # R = G = B
    assert (W, H) == (96, 80) and len(u8) == N and all(np.array_equal(f[:, :, 0], f[:, :, 2]) for f in u8)
    linear = []
    for f in u8:
        x = (ref.srgb_eotf(f / 255.0) / 16.0).astype(np.float32)
        linear.append(np.ascontiguousarray(np.concatenate([x, np.full((H, W, 1), np.nan, np.float32)], axis=2)))
    # channels that differ: B is the clip, R and G are its mirror images
    mixed = [np.ascontiguousarray(np.stack([f[:, ::-1, 0], f[::-1, :, 0], f[:, :, 0]], axis=2)) for f in u8]
    assert not any(np.array_equal(m[:, :, 0], m[:, :, 2]) or np.array_equal(m[:, :, 1], m[:, :, 2]) for m in mixed)
    return {"u8": u8, "linear": linear, "mixed": mixed}


OPTIONS = {"u8": {}, "linear": dict(float_transfer="srgb", float_exposure=4.0), "mixed": dict(channel_weights=(0.0, 0.0, 1.0))}


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _flow_options(core, **kw):
    fo = core.OpticalFlowOptions()
    fo.window_size, fo.max_level = WIN, MAX_LEVEL
    for k, v in kw.items():
        setattr(fo, k, v)
    return fo


def _run(core, path, clip, shard=None, **kw):
    frames = _clips()[clip]
    vi = core.VideoInfo(W, H, 1, N)
    fo = _flow_options(core, **kw)
    if shard is None:
        core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, path, core.GFTTOptions(), fo)
    else:
        core.generate_optical_flow_shard(vi, lambda fid: frames[fid - 1], None, path, shard[0], shard[1], flow_options=fo)
    return _dump(path)


def _run_thread(core, path, clip, **kw):
    frames = _clips()[clip]
    th = core.OpticalFlowThread(core.VideoInfo(W, H, 1, N), path, core.GFTTOptions(), _flow_options(core, **kw))
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
    return _dump(path)


@pytest.fixture(scope="module")
def baseline(core, tmp_path_factory):
    """the database of the uint8 clip under the default options, computed once: what every run below must reproduce"""
    got = _run(core, str(tmp_path_factory.mktemp("gray_conversion") / "u8.db"), "u8")
    k, f = got
    rows = sum(v[0] for v in f.values())
    print("keypoints per frame", [v[0] for _, v in sorted(k.items())], "flow rows", rows)
    assert sorted(k) == list(range(1, N + 1)) and min(v[0] for v in k.values()) >= 20
    assert len(f) == PAIRS and rows >= 10 * PAIRS
    return got


@pytest.mark.parametrize("clip", ["linear", "mixed"])
def test_the_database_call_gives_the_rows_of_the_uint8_clip(core, baseline, tmp_path, clip):
    assert _run(core, str(tmp_path / "a.db"), clip, **OPTIONS[clip]) == baseline
    # ... and the options are what does it: without them the clip gives other rows
    assert _run(core, str(tmp_path / "b.db"), clip) != baseline
    # ... and the parked engine of the runs above carries no conversion over
    assert _run(core, str(tmp_path / "c.db"), "u8") == baseline


@pytest.mark.parametrize("clip", ["linear", "mixed"])
def test_the_thread_gives_the_rows_of_the_uint8_clip(core, baseline, tmp_path, clip):
    assert _run_thread(core, str(tmp_path / "t.db"), clip, **OPTIONS[clip]) == baseline


@pytest.mark.parametrize("clip", ["linear", "mixed"])
def test_two_shards_give_the_one_shard_database(core, baseline, tmp_path, clip):
    k1, f1 = _run(core, str(tmp_path / "s1.db"), clip, shard=(1, 6), **OPTIONS[clip])
    k2, f2 = _run(core, str(tmp_path / "s2.db"), clip, shard=(6, N + 1), **OPTIONS[clip])
    assert sorted(k1) == list(range(1, 6)) and not set(k1) & set(k2)
    assert ({**k1, **k2}, {**f1, **f2}) == baseline


# weights that carry a residual: the largest alone, then each pair of equal largest weights (ties go R, G, B).  Chosen so that the
# residual in another channel changes gray levels of THIS clip (weights with small denominators, (1, 1, 1) or (1, 3, 3), never
# bring a sum within 1 / 32768 of a rounding boundary: their case below checks the rows only)
RESIDUAL_WEIGHTS = [(0.299, 0.587, 0.114), (0.178, 0.586, 0.586), (0.586, 0.586, 0.178), (0.586, 0.178, 0.586)]


@pytest.mark.parametrize("weights", RESIDUAL_WEIGHTS + [(1.0, 1.0, 1.0)], ids=["bt601", "tie_g_b", "tie_r_g", "tie_r_b", "equal"])
def test_weights_whose_quantisation_matters_give_the_rows_of_the_gray_clip_of_the_rule(core, tmp_path, weights):
    """the channels-differ clip under weights that need rounding, a residual and a tie-break, through the driver's quantiser, against
    the clip whose three channels hold ref.gray under ref.quantize(weights): a residual sent to another channel moves gray levels"""
    q = ref.quantize(weights)
    mixed = _clips()["mixed"]
    gray = [ref.gray(f, q) for f in mixed]
    # the rule's plane differs from that of a quantiser that sends the residual elsewhere, truncates, or breaks ties the other way
    s = sum(weights)
    raw = [int(np.floor(c / s * 32768.0 + 0.5)) for c in weights]
    assert sum(raw) != 32768, "the case must carry a residual"
    others = [tuple(raw[k] + (32768 - sum(raw) if k == j else 0) for k in range(3)) for j in range(3)]
    others = [o for o in others if o != q]
    moved = [sum(int((ref.gray(f, o) != g).sum()) for f, g in zip(mixed, gray)) for o in others]
    print(weights, "->", q, "; pixels of the clip that the residual in another channel would change:", moved)
    assert len(others) == 2 and (min(moved) >= 100 or weights not in RESIDUAL_WEIGHTS)
    frames = [np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) for g in gray]
    vi = core.VideoInfo(W, H, 1, N)
    want_path, got_path = str(tmp_path / "want.db"), str(tmp_path / "got.db")
    core.generate_optical_flow_database(vi, lambda fid: frames[fid - 1], None, want_path, core.GFTTOptions(), _flow_options(core))
    want = _dump(want_path)
    assert len(want[1]) == PAIRS and sum(v[0] for v in want[1].values()) >= 10 * PAIRS
    assert _run(core, got_path, "mixed", channel_weights=weights) == want
    assert tuple(core.quantize_channel_weights(weights)) == q


def test_the_transfer_does_nothing_for_uint8_frames_and_the_weights_reach_float_frames(core, baseline, tmp_path):
    assert _run(core, str(tmp_path / "a.db"), "u8", float_transfer="srgb", float_exposure=4.0) == baseline
    assert _run(core, str(tmp_path / "b.db"), "u8", float_transfer="gamma", float_transfer_gamma=2.4, float_exposure=-3.0) == baseline
    # R = G = B: any weights give the channel
    assert _run(core, str(tmp_path / "c.db"), "u8", channel_weights=(0.2, 0.3, 0.5)) == baseline
    assert _run(core, str(tmp_path / "d.db"), "linear", channel_weights=(3.0, 0.0, 1.0), float_transfer="srgb", float_exposure=4.0) == baseline


def test_defaults_give_the_file_of_a_run_that_never_touches_the_options(core, tmp_path, monkeypatch):
    # one transaction per frame, so that whole files can be compared (tests/test_lk_fb_gpu.py explains)
    monkeypatch.setenv("POLYCHASE_DB_BATCH_FRAMES", "1")
    a, b, c = (str(tmp_path / n) for n in ("untouched.db", "defaults.db", "on.db"))
    _run(core, a, "mixed")
    _run(core, b, "mixed", channel_weights=None, float_transfer="none", float_transfer_gamma=2.2, float_exposure=0.0)
    assert open(a, "rb").read() == open(b, "rb").read()
    _run(core, c, "mixed", **OPTIONS["mixed"])
    assert _dump(c) != _dump(a)
    _run(core, b + "2", "mixed")      # the parked engine of the run above carries nothing over
    assert open(b + "2", "rb").read() == open(a, "rb").read()


def test_a_resumed_run_keeps_the_rows_already_stored(core, baseline, tmp_path):
    path = str(tmp_path / "resumed.db")
    k1, f1 = _run(core, path, "mixed", shard=(1, 6))                         # default conversion: other rows than the baseline's
    assert any(f1[p] != baseline[1][p] for p in f1)
    k, f = _run(core, path, "mixed", **OPTIONS["mixed"])                      # the rest under (0, 0, 1)
    assert all(k[i] == k1[i] for i in k1) and all(f[p] == f1[p] for p in f1)
    assert all(k[i] == baseline[0][i] for i in range(6, N + 1))
