"""GPU: uint16, float16 and RGBA frames through polychase_core.  Whatever the hand-over -- generate_optical_flow_database with
numpy frames, OpticalFlowThread.provide_frame, torch device tensors -- the database is, byte for byte,

  * of the uint16 clip x * 257 and of the uint8 RGBA clip with random alpha: the uint8 clip's;
  * of a float16 clip h: the float32 clip h.astype(float32)'s, without a transfer curve and under float_transfer = "srgb"."""
import functools
import os
import sqlite3
import sys
import time

import numpy as np
import pytest

import ingest_layouts as il
from polychase_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 157, 93, 10          # w mod 4 = 1: no row of any pixel type here is a multiple of 4 bytes but RGBA's
SRGB = dict(float_transfer="srgb", float_exposure=0.0)


@pytest.fixture(scope="module")
def core():
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@functools.lru_cache(maxsize=None)
def _clips():
    clip = synth.NoiseClip(W, H, N)
    u8 = [np.ascontiguousarray(clip.frame(t)) for t in range(N)]
    rng = np.random.default_rng(16)
    u16 = [f.astype(np.uint16) * np.uint16(257) for f in u8]
    rgba8 = [np.ascontiguousarray(np.concatenate([f, rng.integers(0, 256, (H, W, 1), dtype=np.uint8)], axis=2)) for f in u8]
    # halves of [0, 1] that follow the clip (so that there is something to track), with an alpha of NaNs
    f16 = []
    for f in u8:
        x = ((f.astype(np.float32) + rng.uniform(0.05, 0.95, f.shape).astype(np.float32)) / np.float32(255.0)).astype(np.float16)
        assert x.min() >= 0 and x.max() <= 1
        f16.append(np.ascontiguousarray(np.concatenate([x, np.full((H, W, 1), np.nan, np.float16)], axis=2)))
    f32 = [h.astype(np.float32) for h in f16]
    assert not np.array_equal(il.float_to_u8(f32[0][:, :, :3]), u8[0])       # rounding to half moved bytes: a clip of its own
    return {"u8": u8, "u16": u16, "rgba8": rgba8, "f16": f16, "f32": f32}


def _dump(path):
    con = sqlite3.connect(path)
    k = {r[0]: (r[1], bytes(r[2] or b"")) for r in con.execute("select image_id, rows, keypoints from keypoints")}
    f = {(r[0], r[1]): (r[2],) + tuple(bytes(b or b"") for b in r[3:]) for r in con.execute(
        "select image_id_from, image_id_to, rows, src_keypoints_indices, tgt_keypoints, flow_errors from optical_flow")}
    con.close()
    return k, f


def _flow_options(core, **kw):
    fo = core.OpticalFlowOptions()
    for k, v in kw.items():
        setattr(fo, k, v)
    return fo


def _run(core, path, frames, **kw):
    core.generate_optical_flow_database(core.VideoInfo(W, H, 1, N), lambda fid: frames[fid - 1], None, path, core.GFTTOptions(),
                                        _flow_options(core, **kw))
    return _dump(path)


def _run_thread(core, path, frames, **kw):
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
def baselines(core, tmp_path_factory):
    """the databases the new pixel types must reproduce, each computed once from frames of the types the library always took"""
    d = tmp_path_factory.mktemp("ingest16")
    out = {"u8": _run(core, str(d / "u8.db"), _clips()["u8"]), "f32": _run(core, str(d / "f32.db"), _clips()["f32"]),
           "f32_srgb": _run(core, str(d / "f32s.db"), _clips()["f32"], **SRGB)}
    for k, f in out.values():
        assert len(k) == N and min(v[0] for v in k.values()) > 20 and sum(v[0] for v in f.values()) > 20 * N
    assert out["u8"] != out["f32"] and out["f32"] != out["f32_srgb"]
    return out


def test_uint16_clip_gives_the_uint8_clips_database(core, baselines, tmp_path):
    assert _run(core, str(tmp_path / "a.db"), _clips()["u16"]) == baselines["u8"]


def test_rgba_bytes_give_the_uint8_clips_database(core, baselines, tmp_path):
    assert _run(core, str(tmp_path / "a.db"), _clips()["rgba8"]) == baselines["u8"]


@pytest.mark.parametrize("curve", ["none", "srgb"])
def test_float16_clip_gives_its_float32_widenings_database(core, baselines, tmp_path, curve):
    kw, want = (SRGB, baselines["f32_srgb"]) if curve == "srgb" else ({}, baselines["f32"])
    assert _run(core, str(tmp_path / "a.db"), _clips()["f16"], **kw) == want


@pytest.mark.parametrize("clip,want,kw", [("u16", "u8", {}), ("rgba8", "u8", {}), ("f16", "f32", {}), ("f16", "f32_srgb", SRGB)],
                         ids=["uint16", "rgba8", "float16", "float16_srgb"])
def test_through_provide_frame(core, baselines, tmp_path, clip, want, kw):
    assert _run_thread(core, str(tmp_path / "a.db"), _clips()[clip], **kw) == baselines[want]


@pytest.mark.parametrize("clip,want,kw", [("u16", "u8", {}), ("rgba8", "u8", {}), ("f16", "f32", {}), ("f16", "f32_srgb", SRGB)],
                         ids=["uint16", "rgba8", "float16", "float16_srgb"])
def test_as_torch_device_tensors(core, baselines, tmp_path, clip, want, kw):
    import torch
    frames = _clips()[clip]
    if clip == "u16":
        # torch.uint16 where the installed torch has it (the issue's wording); the same bytes travel either way
        assert hasattr(torch, "uint16"), "this torch has no uint16: the hand-over cannot be made"
        dev = [torch.from_numpy(f.view(np.int16)).cuda().view(torch.uint16) for f in frames]
    else:
        dev = [torch.from_numpy(f).cuda() for f in frames]
    assert _run(core, str(tmp_path / "a.db"), dev, **kw) == baselines[want]


def test_other_frames_are_a_value_error(core, tmp_path):
    for bad in (np.zeros((H, W, 3), np.int16), np.zeros((H, W, 3), np.float64), np.zeros((H, W, 2), np.uint16), np.zeros((H, W), np.uint16)):
        with pytest.raises(ValueError, match="uint16"):
            _run(core, str(tmp_path / "bad.db"), [bad] * N)
