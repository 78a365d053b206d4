"""Lens undistortion at ingest (include/polychase_hip.h: pc_lens_model, pc_context_set_lens_map) restated in numpy.  TEST
INFRASTRUCTURE ONLY; nothing here needs a GPU or the library.

  build_map(model, w, h)        polynomial model -> int32 (h, w, 2), fp64, the header's operations in the header's order
  map_from_stmap(st, flip_v)    float32 STmap -> map
  quantize(sx, sy)              source positions -> map entries (floor(s * 256 + 0.5), clamp +-2^24, non-finite -> INVALID pair)
  remap(gray, q)                the bilinear blend in int64
  valid(q, erode)               the validity plane 255 / 0 and its box erosion (brute force over the box)
  model(...)                    a dict with the ten fields; pincushion(w, h) etc.: the models the tests share
  scene helpers                 texture(), sample(), distort_points(): the recipe scene of tests/test_lens_cpu.py
"""
from __future__ import annotations

import numpy as np

FRAC_BITS = 8
INVALID = -2 ** 31
CLAMP = 2 ** 24
FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2", "zoom")


def model(fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0, zoom=1.0) -> dict:
    return dict(zip(FIELDS, (float(v) for v in (fx, fy, cx, cy, k1, k2, k3, p1, p2, zoom))))


def recipe_model(w=320, h=240, f=300.0) -> dict:
    """the barrel lens of the recipe scene, principal point at the centre of a w x h frame"""
    return model(f, f, (w - 1) / 2.0, (h - 1) / 2.0, k1=-0.15, k2=0.02, p1=0.001, p2=-0.0005)


def pincushion(w, h) -> dict:
    """k1 = +0.15, k2 = 0.05 with the focal length scaled to the size: the corners of the undistorted frame leave the original"""
    return model(0.9375 * w, 0.9375 * w, (w - 1) / 2.0, (h - 1) / 2.0, k1=0.15, k2=0.05)


def quantize(sx: np.ndarray, sy: np.ndarray) -> np.ndarray:
    sx, sy = np.asarray(sx, np.float64), np.asarray(sy, np.float64)
    bad = ~(np.isfinite(sx) & np.isfinite(sy))
    out = np.empty(sx.shape + (2,), np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, s in enumerate((sx, sy)):
            v = np.floor(np.where(bad, 0.0, s) * 256.0 + 0.5)
            out[..., k] = np.clip(v, -float(CLAMP), float(CLAMP)).astype(np.int64)
    out[bad] = INVALID
    return out


def source_positions(m: dict, w: int, h: int):
    """(sx, sy) float64 (h, w): every operation a separate rounded fp64 operation, in the header's order"""
    fx, fy, cx, cy, k1, k2, k3, p1, p2, zoom = (np.float64(m[k]) for k in FIELDS)
    u = np.arange(w, dtype=np.float64)[None, :]
    v = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.broadcast_to((u - cx) / (fx * zoom), (h, w))
        y = np.broadcast_to((v - cy) / (fy * zoom), (h, w))
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        sx = xd * fx + cx
        sy = yd * fy + cy
    return sx, sy


def build_map(m: dict, w: int, h: int) -> np.ndarray:
    return quantize(*source_positions(m, w, h))


def map_from_stmap(st: np.ndarray, flip_v: bool = True) -> np.ndarray:
    st = np.asarray(st)
    assert st.dtype == np.float32 and st.ndim == 3 and st.shape[2] == 2
    h, w = st.shape[:2]
    s, t = st[..., 0].astype(np.float64), st[..., 1].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sx = s * np.float64(w) - 0.5
        sy = ((1.0 - t) * np.float64(h) - 0.5) if flip_v else (t * np.float64(h) - 0.5)
    return quantize(sx, sy)


def identity_map(w: int, h: int) -> np.ndarray:
    q = np.empty((h, w, 2), np.int32)
    q[..., 0] = 256 * np.arange(w)[None, :]
    q[..., 1] = 256 * np.arange(h)[:, None]
    return q


def remap(gray: np.ndarray, q: np.ndarray) -> np.ndarray:
    gray = np.asarray(gray)
    assert gray.dtype == np.uint8 and gray.ndim == 2 and q.dtype == np.int32 and q.shape == gray.shape + (2,)
    h, w = gray.shape
    g = gray.astype(np.int64)
    qx, qy = q[..., 0].astype(np.int64), q[..., 1].astype(np.int64)
    bad = (qx == INVALID) | (qy == INVALID)
    ix, iy = qx >> FRAC_BITS, qy >> FRAC_BITS          # arithmetic shifts: floor
    wx, wy = qx & 255, qy & 255
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    a, b, c, d = g[y0, x0], g[y0, x1], g[y1, x0], g[y1, x1]
    top = a * (256 - wx) + b * wx
    bot = c * (256 - wx) + d * wx
    out = (top * (256 - wy) + bot * wy + 32768) >> 16
    out[bad] = 0
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def valid(q: np.ndarray, erode: int = 0) -> np.ndarray:
    h, w = q.shape[:2]
    qx, qy = q[..., 0].astype(np.int64), q[..., 1].astype(np.int64)
    ok = (qx >= 0) & (qx <= (w - 1) * 256) & (qy >= 0) & (qy <= (h - 1) * 256)
    out = ok.copy()
    m = int(erode)
    # a pixel stays on iff every pixel of the box that lies inside the frame is valid: shifts that leave the frame judge nothing
    for dy in range(-m, m + 1):
        for dx in range(-m, m + 1):
            if abs(dy) >= h or abs(dx) >= w:
                continue
            ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            out[yd, xd] &= ok[ys, xs]
    return np.where(out, 255, 0).astype(np.uint8)


# ---- the recipe scene -----------------------------------------------------------------------------------------------
def texture(seed: int = 1, n: int = 60):
    """60 sinusoids, 0.02 .. 0.22 cycles / px per axis with random sign, amplitude 0.5 .. 1 -> a function (x, y) -> float; the
    values are scaled to +-100 about 128 by sample()"""
    rng = np.random.default_rng(seed)
    fx = rng.uniform(0.02, 0.22, n) * rng.choice([-1.0, 1.0], n)
    fy = rng.uniform(0.02, 0.22, n) * rng.choice([-1.0, 1.0], n)
    amp = rng.uniform(0.5, 1.0, n)
    ph = rng.uniform(0, 2 * np.pi, n)

    def f(x, y):
        acc = np.zeros(np.broadcast(x, y).shape, np.float64)
        for k in range(n):
            acc += amp[k] * np.sin(2 * np.pi * (fx[k] * x + fy[k] * y) + ph[k])
        return acc

    # the scale: the largest magnitude over a generous area, so that every frame of a scene shares it
    xs, ys = np.meshgrid(np.arange(-40.0, 400.0, 1.0), np.arange(-40.0, 320.0, 1.0))
    peak = float(np.abs(f(xs, ys)).max())
    return lambda x, y: f(x, y) / peak


def sample(tex, x, y, shift=(0.0, 0.0)) -> np.ndarray:
    """the texture moved by `shift` (content at p appears at p + shift), sampled at (x, y): +-100 about 128, rounded -> u8"""
    return np.clip(np.rint(128.0 + 100.0 * tex(x - shift[0], y - shift[1])), 0, 255).astype(np.uint8)


def distort_points(m: dict, u, v):
    """undistorted pixel positions (float) -> positions in the original frame, by the model (plain fp64, for scenes)"""
    x = (u - m["cx"]) / (m["fx"] * m["zoom"])
    y = (v - m["cy"]) / (m["fy"] * m["zoom"])
    r2 = x * x + y * y
    rad = 1.0 + r2 * (m["k1"] + r2 * (m["k2"] + r2 * m["k3"]))
    xd = x * rad + 2.0 * m["p1"] * x * y + m["p2"] * (r2 + 2.0 * x * x)
    yd = y * rad + m["p1"] * (r2 + 2.0 * y * y) + 2.0 * m["p2"] * x * y
    return xd * m["fx"] + m["cx"], yd * m["fy"] + m["cy"]


def undistort_points(m: dict, sx, sy, iters: int = 30):
    """positions in the original frame -> undistorted pixel positions: the fixed-point iteration of the model's inverse"""
    xd, yd = (sx - m["cx"]) / m["fx"], (sy - m["cy"]) / m["fy"]
    x, y = xd.copy(), yd.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (m["k1"] + r2 * (m["k2"] + r2 * m["k3"]))
        dx = 2.0 * m["p1"] * x * y + m["p2"] * (r2 + 2.0 * x * x)
        dy = m["p1"] * (r2 + 2.0 * y * y) + 2.0 * m["p2"] * x * y
        x, y = (xd - dx) / rad, (yd - dy) / rad
    return x * (m["fx"] * m["zoom"]) + m["cx"], y * (m["fy"] * m["zoom"]) + m["cy"]


def scene_frames(w, h, m, shifts, seed=1):
    """-> (pinhole frames, distorted frames) u8 (h, w) for every shift: the pinhole frame samples the shifted texture at its own
    pixels, the distorted frame at the undistorted position of each of its pixels (what a camera with the lens records).  A crop
    of the recipe scene is the recipe model with its principal point moved by the crop's offset"""
    tex = texture(seed)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ux, uy = undistort_points(m, xs, ys)
    pin = [sample(tex, xs, ys, s) for s in shifts]
    dist = [sample(tex, ux, uy, s) for s in shifts]
    return pin, dist
