"""Scenes of the minimum-correlation tests (tests/test_lk_correlation_cpu.py, tests/test_lk_correlation_gpu.py).  TEST
INFRASTRUCTURE ONLY.

96 x 80 gray frames from tests/fb_scene.py: frame 1 is the texture of seed 11; a target is it unchanged ('same'), shifted by a
sub-pixel amount with an occluder ('shift'; the `far` shift above window 16), that under a global gain and bias ('gain':
x 0.6 + 40, the exposure change the patch error cannot tell from drift), unrelated texture, or shifted towards the lower right
so that rows end outside the frame ('border')."""
from __future__ import annotations

import functools

import numpy as np

import fb_scene
import oracle

W, H = 96, 80
BASE_SEED, TARGET_SEED = 11, 5
WINDOWS = (3, 10, 21, 31)
MIX8 = ("same", "shift", "gain", "unrelated", "border", "shift", "gain", "border")


def gain(gray: np.ndarray, a: float = 0.6, b: float = 40.0) -> np.ndarray:
    return fb_scene.to_u8(gray.astype(np.float64) * a + b)


@functools.lru_cache(maxsize=None)
def frame1() -> np.ndarray:
    g = fb_scene.to_u8(fb_scene.texture(W, H, BASE_SEED))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def target(kind: str, win: int, seed: int = TARGET_SEED) -> np.ndarray:
    base = fb_scene.texture(W, H, BASE_SEED)
    far = win > 16
    g = gain(fb_scene.target(base, "shift", seed, far)) if kind == "gain" else fb_scene.target(base, kind, seed, far)
    g.setflags(write=False)
    return g


def targets(win: int, count: int):
    """the first `count` of the mix of eight; the second round of kinds takes other seeds"""
    return [target(k, win, TARGET_SEED if i < 5 else TARGET_SEED + 7 * i) for i, k in enumerate(MIX8[:count])]


@functools.lru_cache(maxsize=None)
def detected() -> np.ndarray:
    k = oracle.gftt(frame1())
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def keypoints(win: int) -> np.ndarray:
    """the detector's keypoints, then sub-pixel ones, ones within a window of the border, and ones outside the frame (the last
    four so far out that the template window fails the bounds test)"""
    k = detected()
    frac = np.array([(0.25, 0.5), (0.73, -0.31), (-0.5, 0.125), (0.999, 0.001)], np.float32)
    sub = k[:24] + frac[np.arange(24) % len(frac)]
    border = [(1.5, 40.0), (W - 2.25, 30.5), (50.25, 0.75), (47.0, H - 1.5), (0.0, 0.0), (W - 1.0, H - 1.0), (win / 2.0, win / 2.0),
              (W - 1.0 - win / 2.0, 20.3), (win - 0.5, H - win + 0.25)]
    outside = [(-3.5, 20.0), (W + 2.0, 30.25), (40.5, -2.75), (30.0, H + 1.5), (-(win / 2.0) - 0.25, 33.0),
               (-(win + 6.0), 10.0), (W + win + 3.0, 10.0), (20.0, -(win + 8.0)), (20.0, H + win + 2.0)]
    out = np.ascontiguousarray(np.concatenate([k, sub, np.array(border, np.float32), np.array(outside, np.float32)]), np.float32)
    out.setflags(write=False)
    return out


def check_fractions(forward: int, kept: int, what=""):
    """the scene must exercise both outcomes: asserted on the REFERENCE's result, before anything is compared with it"""
    assert forward >= 10, (what, forward)
    assert forward - kept >= 0.1 * forward, (what, forward, kept)
    assert kept >= 0.1 * forward, (what, forward, kept)
