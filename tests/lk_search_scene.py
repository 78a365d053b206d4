"""Scenes of the search prepass tests (tests/test_lk_search_gpu.py, tests/test_lk_search_product_gpu.py).  TEST INFRASTRUCTURE ONLY.

160 x 120 gray frames cut from one texture, fb_scene.to_u8(fb_scene.texture(W + 160, H + 160, 11)): frame1 is the crop at (80, 80),
a displaced target the crop at (80 - dx, 80 - dy), so keypoint p of frame1 lies at p + (dx, dy) there.  Eight targets mix the
unchanged frame, displacements the plain search reaches ((5, -3)), half reaches ((19, -11)) and loses ((37, -22)), unrelated
texture and a flat plane.  73 keypoints: detected corners, some moved off the pixel grid, points within 4 * 2^s pixels of each
border for every search level s the tests reach, and points outside the frame; 73 leaves the last workgroup of every launch
partly filled.  The reference of a (window, radius, arithmetic mode, fb threshold) is computed once and shared."""
from __future__ import annotations

import functools

import numpy as np

import fb_scene
import lk_search_ref as ref
import oracle

W, H, MAX_LEVEL = 160, 120, 2
MIX8 = ("same", (19, -11), (37, -22), "unrelated", "flat", (-19, 11), (5, -3), (-37, 22))


@functools.lru_cache(maxsize=None)
def canvas() -> np.ndarray:
    c = fb_scene.to_u8(fb_scene.texture(W + 160, H + 160, 11))
    c.setflags(write=False)
    return c


def crop(dx=0, dy=0) -> np.ndarray:
    return np.ascontiguousarray(canvas()[80 - dy:80 - dy + H, 80 - dx:80 - dx + W])


def frame1() -> np.ndarray:
    return crop()


def target(kind) -> np.ndarray:
    if kind == "same":
        return crop()
    if kind == "unrelated":
        return fb_scene.to_u8(fb_scene.texture(W, H, 23))
    if kind == "flat":
        return np.full((H, W), 117, np.uint8)
    return crop(*kind)


def targets(count=8):
    return [target(k) for k in MIX8[:count]]


@functools.lru_cache(maxsize=None)
def keypoints() -> np.ndarray:
    with oracle.emulation(oracle.EMU_CANONICAL):
        det = oracle.gftt(frame1())
    det = det[::max(1, len(det) // 49)][:49].copy()
    det[::3] += np.float32([0.25, 0.625])          # off the pixel grid
    det[1::5] -= np.float32([0.5, 0.125])
    edge = [(3.5, 60.0), (4.0, 30.25), (7.75, 90.0), (15.0, 61.5), (19.5, 20.0), (156.25, 60.0), (155.5, 33.0), (152.0, 91.5), (145.5, 46.25),
            (145.5, 52.25), (80.0, 2.0), (41.5, 4.0), (120.0, 7.5), (81.0, 14.5), (60.0, 19.75), (80.0, 117.0), (40.25, 115.5), (119.0, 112.0),
            (82.5, 105.0), (61.0, 100.5)]
    outside = [(-5.0, 50.0), (170.0, 50.5), (80.0, -3.0), (80.25, 125.0)]
    pts = np.concatenate([det, np.array(edge + outside, np.float32)]).astype(np.float32)
    assert len(pts) == 73, len(pts)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def pyramids(win: int):
    """canonical pyramids (the image and derivative planes do not depend on the LK order) of frame1 and of the eight targets"""
    with oracle.emulation(oracle.EMU_CANONICAL):
        return oracle.Pyramid(frame1(), win, MAX_LEVEL), [oracle.Pyramid(t, win, MAX_LEVEL) for t in targets()]


@functools.lru_cache(maxsize=None)
def forward(win: int, emu: int):
    """the forward rows of the eight targets in the given emulation"""
    p1, pts = pyramids(win)
    opt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    with oracle.emulation(emu):
        return [oracle.lk(p1, pt, keypoints(), opt) for pt in pts]


@functools.lru_cache(maxsize=None)
def reference(win: int, R: int, emu: int, fb: float = 0.0):
    """per target (next_xy, status, err, search_d, search_state, back_xy, back_status); with fb > 0 the status is the final one, else
    the back arrays are zero"""
    p1, pts = pyramids(win)
    P, Ns = ref.Planes(p1), [ref.Planes(p) for p in pts]
    opt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    kps = keypoints()
    rows = ref.search(P, Ns, kps, forward(win, emu), opt, R)
    out = []
    for pt, N, row in zip(pts, Ns, rows):
        bxy, bst, st = np.zeros((len(kps), 2), np.float32), np.zeros(len(kps), np.uint8), row[1]
        if fb > 0:
            def plain_back(q):
                with oracle.emulation(emu):
                    b, sb, _ = oracle.lk(pt, p1, q, opt)
                return b, sb
            st, bxy, bst = ref.backward(P, N, kps, row, opt, fb, plain_back)
        out.append((row[0], st, row[2], row[3], row[4], bxy, bst))
    return out


def clip(n: int, step: int = 12):
    """n RGB frames (R = G = B) panning by `step` pixels per frame: frame t shows the canvas displaced by (-t * step, 0)"""
    return [np.ascontiguousarray(np.repeat(crop(-(t - n // 2) * step, 0)[:, :, None], 3, axis=2)) for t in range(n)]
