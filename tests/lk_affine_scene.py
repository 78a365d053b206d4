"""Scenes of the affine refinement tests (tests/test_lk_affine_cpu.py, tests/test_lk_affine_gpu.py).  TEST INFRASTRUCTURE ONLY.

96 x 80 gray frames.  Frame 1 is the centre of tests/fb_scene.py's texture of seed 11 drawn on a canvas 24 px larger per side; a
similarity target is that canvas resampled (bilinear, float64) under a rotation and a zoom about the frame centre plus a shift
of (2.3, -1.7) px -- 'rot' 8 degrees, 'zoom' x 1.10, 'sim' 4 degrees and x 1.05 -- and comes with its analytic flow.  The other
targets are fb_scene.target's of frame 1: 'same', 'shift', 'border', 'unrelated' (the `far` shift above window 16).  The keypoints
are built as tests/lk_correlation_scene.py builds its own: the detector's, sub-pixel ones, ones within a window of the border and
ones outside the frame."""
from __future__ import annotations

import functools
import math

import numpy as np

import fb_scene
import lk_correlation_scene as cscene
import oracle

W, H, MARGIN = 96, 80, 24
BASE_SEED, TARGET_SEED = 11, 5
SHIFT = (2.3, -1.7)
SIMILARITIES = {"rot": (8.0, 1.0), "zoom": (0.0, 1.10), "sim": (4.0, 1.05)}        # degrees, scale
MIX7 = ("rot", "zoom", "sim", "same", "shift", "border", "unrelated")
MIX8 = MIX7 + ("sim",)
CENTRE = ((W - 1) * 0.5, (H - 1) * 0.5)


@functools.lru_cache(maxsize=None)
def canvas() -> np.ndarray:
    c = fb_scene.texture(W + 2 * MARGIN, H + 2 * MARGIN, BASE_SEED)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def base() -> np.ndarray:
    """frame 1 before rounding, float64"""
    b = np.ascontiguousarray(canvas()[MARGIN:MARGIN + H, MARGIN:MARGIN + W])
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def frame1() -> np.ndarray:
    g = fb_scene.to_u8(base())
    g.setflags(write=False)
    return g


def _matrix(kind):
    """kind: a key of SIMILARITIES or (degrees, scale)"""
    deg, s = SIMILARITIES[kind] if isinstance(kind, str) else kind
    c, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[s * c, -s * sn], [s * sn, s * c]])


def flow(kind: str, pts: np.ndarray) -> np.ndarray:
    """the analytic end points of `pts` [N, 2] in a similarity target: x' = centre + A (x - centre) + SHIFT, float64"""
    p = np.asarray(pts, np.float64) - CENTRE
    return p @ _matrix(kind).T + CENTRE + SHIFT


def _similarity(kind, shift=SHIFT) -> np.ndarray:
    inv = np.linalg.inv(_matrix(kind))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = xs - CENTRE[0] - shift[0], ys - CENTRE[1] - shift[1]
    sx = inv[0, 0] * dx + inv[0, 1] * dy + CENTRE[0] + MARGIN           # canvas coordinates of every target pixel
    sy = inv[1, 0] * dx + inv[1, 1] * dy + CENTRE[1] + MARGIN
    c = canvas()
    assert sx.min() >= 0 and sy.min() >= 0 and sx.max() < c.shape[1] - 1 and sy.max() < c.shape[0] - 1, "the canvas covers the target"
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    fx, fy = sx - x0, sy - y0
    top = c[y0, x0] * (1 - fx) + c[y0, x0 + 1] * fx
    bot = c[y0 + 1, x0] * (1 - fx) + c[y0 + 1, x0 + 1] * fx
    return top * (1 - fy) + bot * fy


@functools.lru_cache(maxsize=None)
def target(kind: str, win: int, seed: int = TARGET_SEED) -> np.ndarray:
    g = fb_scene.to_u8(_similarity(kind)) if kind in SIMILARITIES else fb_scene.target(np.array(base()), kind, seed, win > 16)
    g.setflags(write=False)
    return g


def rolling_clip(n: int, degrees_per_frame: float = 1.5):
    """n RGB uint8 frames (R = G = B): the canvas under a roll of `degrees_per_frame` per frame about the frame centre and a drift of
    (0.75, -0.5) px per frame"""
    assert (n - 1) * degrees_per_frame <= 8.0, "the canvas covers 8 degrees"
    return [np.ascontiguousarray(np.repeat(fb_scene.to_u8(_similarity((degrees_per_frame * t, 1.0), (0.75 * t, -0.5 * t)))[:, :, None], 3, axis=2))
            for t in range(n)]


def targets(win: int, count: int):
    """the first `count` of the mix of eight"""
    return [target(k, win) for k in MIX8[:count]]


@functools.lru_cache(maxsize=None)
def detected() -> np.ndarray:
    k = oracle.gftt(frame1())
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def keypoints(win: int) -> np.ndarray:
    """lk_correlation_scene.keypoints' recipe on this scene's frame 1 (same size): the detector's keypoints, 24 sub-pixel ones, 9
    within a window of the border, 9 outside the frame (the last four so far out that the template window fails the bounds test)"""
    assert (W, H) == (cscene.W, cscene.H)
    tail = cscene.keypoints(win)[len(cscene.detected()) + 24:]
    k = detected()
    frac = np.array([(0.25, 0.5), (0.73, -0.31), (-0.5, 0.125), (0.999, 0.001)], np.float32)
    sub = k[:24] + frac[np.arange(24) % len(frac)]
    out = np.ascontiguousarray(np.concatenate([k, sub, tail]), np.float32)
    out.setflags(write=False)
    return out


def interior(pts: np.ndarray, win: int) -> np.ndarray:
    """boolean: more than win + 4 px from every border"""
    pts = np.asarray(pts)
    return (pts[:, 0] > win + 4) & (pts[:, 0] < W - 1 - (win + 4)) & (pts[:, 1] > win + 4) & (pts[:, 1] < H - 1 - (win + 4))


MAX_LEVEL = 2


@functools.lru_cache(maxsize=None)
def reference(win: int, kinds: tuple = MIX7, emu: int = oracle.EMU_CANONICAL):
    """the oracle's forward rows of `kinds` under emulation `emu` and the rule's refinement of them (tests/lk_affine_ref.py), computed
    once and shared: -> (keypoints, forward, refined), the latter two lists per target of (next_xy, status, err) and of
    (next_xy, status, err, affine_m, affine_state).  Read-only."""
    import lk_affine_ref as ref

    kps = keypoints(win)
    opt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    with oracle.emulation(emu):
        p1 = oracle.Pyramid(np.array(frame1()), win, MAX_LEVEL)
        pts = [oracle.Pyramid(np.array(target(k, win)), win, MAX_LEVEL) for k in kinds]
        forward = [oracle.lk(p1, pt, kps, opt) for pt in pts]
    refined = ref.refine(ref.Planes(p1), [ref.Planes(p) for p in pts], kps, forward, opt)
    for rows in forward + refined:
        for a in rows:
            a.setflags(write=False)
    return kps, forward, refined
