"""The two-layer scene of the masked-window tests: a textured disc (the foreground, the matted object) that moves one way over a
textured background that moves another.  TEST INFRASTRUCTURE ONLY.

Both layers are band-limited noise: a seeded integer field, box-blurred three times with exact integer sums, sampled bilinearly in
float64 at the layer's displacement (plain IEEE adds and multiplies: the same bytes on every machine).  The mask of a frame is
its disc.  Keypoints for the effect measurement lie on rings inside the outline of frame 0's disc; their true motion is the
foreground's."""
from __future__ import annotations

import numpy as np

W, H = 192, 160
CENTRE = (96.0, 80.0)
RADIUS = 56.0
FG_MOTION = (-2.0, 1.5)
BG_MOTION = (3.0, 0.5)
_PAD = 16


def _texture(seed, blur):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, size=(H + 2 * _PAD + 6 * blur, W + 2 * _PAD + 6 * blur)).astype(np.int64)
    for _ in range(3):   # three box passes of width 2 blur + 1, exact integers
        c = np.cumsum(np.pad(a, ((1, 0), (0, 0))), axis=0)
        a = c[2 * blur + 1:] - c[:-(2 * blur + 1)]
        c = np.cumsum(np.pad(a, ((0, 0), (1, 0))), axis=1)
        a = c[:, 2 * blur + 1:] - c[:, :-(2 * blur + 1)]
    lo, hi = int(a.min()), int(a.max())
    return ((a - lo) * 255 // (hi - lo)).astype(np.float64)   # (H + 2 PAD, W + 2 PAD), 0 .. 255


def _sample(tex, dx, dy):
    """the layer displaced by (dx, dy): out(x, y) = tex(x - dx, y - dy), bilinear"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    sx, sy = xs - dx + _PAD, ys - dy + _PAD
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    a, b = sx - x0, sy - y0
    return (tex[y0, x0] * (1 - a) * (1 - b) + tex[y0, x0 + 1] * a * (1 - b) + tex[y0 + 1, x0] * (1 - a) * b + tex[y0 + 1, x0 + 1] * a * b)


def disc(k=0):
    """the mask of frame k: uint8 (H, W), 255 inside the disc"""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy = CENTRE[0] + k * FG_MOTION[0], CENTRE[1] + k * FG_MOTION[1]
    return (((xs - cx) ** 2 + (ys - cy) ** 2 <= RADIUS ** 2) * 255).astype(np.uint8)


def frame(k, seed=7):
    """the scene at time k (|k| <= 4, fractions allowed) -> gray uint8 (H, W), its mask"""
    f = _sample(_texture(seed, 2), k * FG_MOTION[0], k * FG_MOTION[1])
    b = _sample(_texture(seed + 1, 2), k * BG_MOTION[0], k * BG_MOTION[1])
    return np.where(disc(k) != 0, f, b).round().astype(np.uint8), disc(k)


def frames(seed=7):
    """-> (gray0, gray1) uint8 (H, W), (mask0, mask1)"""
    (g0, m0), (g1, m1) = frame(0, seed), frame(1, seed)
    return (g0, g1), (m0, m1)


def ring_keypoints(depth_lo, depth_hi, n=40):
    """n keypoints inside frame 0's outline, depths spread evenly over (depth_lo, depth_hi], angles evenly around the disc"""
    k = np.arange(n, dtype=np.float64)
    depth = depth_lo + (depth_hi - depth_lo) * (k + 1) / n
    ang = 2.0 * np.pi * (k * 7 % n) / n + 0.1
    r = RADIUS - depth
    return np.stack([CENTRE[0] + r * np.cos(ang), CENTRE[1] + r * np.sin(ang)], axis=1).astype(np.float32)


def truth(pts):
    return np.asarray(pts, np.float64) + np.array(FG_MOTION)
