"""Scenes and the CPU composition for the forward-backward check of the LK flow (tests/test_lk_fb_gpu.py).  TEST INFRASTRUCTURE ONLY.

Images: box-blurred seeded noise (numpy only).  A target is frame 1 shifted by a sub-pixel amount with a rectangle of about a
third of each side replaced by unrelated texture: keypoints outside the rectangle track there and back, keypoints inside it
(and windows that straddle its edge) do not.

The expected result is the oracle composed with itself:
    q, status_f, err = oracle.lk(p1, pT, kps);  b, status_b = oracle.lk(pT, p1, q[status_f == 1])
    keep = status_f == 1 and status_b == 1 and d2 <= thr2      (include/polychase_hip.h: pc_lk_track_fb)
with d2 in separately rounded float32 operations and thr2 = float32(float64(thr) * float64(thr))."""
from __future__ import annotations

import numpy as np

import oracle


def texture(w: int, h: int, seed: int, blur: int = 3) -> np.ndarray:
    """float64 (h, w) in 0..255: seeded uniform noise under a blur x blur box filter, contrast stretched"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 255.0, (h + blur - 1, w + blur - 1))
    c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), axis=0), axis=1)
    s = (c[blur:, blur:] - c[:-blur, blur:] - c[blur:, :-blur] + c[:-blur, :-blur]) / (blur * blur)
    return np.clip((s - 127.5) * 2.0 + 127.5, 0.0, 255.0)


def shifted(img: np.ndarray, dx: float, dy: float) -> np.ndarray:
    """out(x, y) = img(x - dx, y - dy), bilinear, edge pixels repeated"""
    h, w = img.shape
    x = np.clip(np.arange(w) - dx, 0, w - 1)
    y = np.clip(np.arange(h) - dy, 0, h - 1)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (x - x0)[None, :], (y - y0)[:, None]
    top = img[y0][:, x0] * (1 - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (1 - fx) + img[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def to_u8(img: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def occluded(img: np.ndarray, seed: int, x0: float = 0.3, y0: float = 0.3) -> np.ndarray:
    """a rectangle of a third of each side, its corner at (x0, y0) of the size, replaced by unrelated texture"""
    h, w = img.shape
    out = img.copy()
    rw, rh, rx, ry = w // 3, h // 3, int(w * x0), int(h * y0)
    out[ry:ry + rh, rx:rx + rw] = texture(rw, rh, seed)
    return out


def target(base: np.ndarray, kind: str, seed: int, far: bool = False) -> np.ndarray:
    """uint8 gray target of `base` (float): 'shift' (3.25, -2.5) px + occluder -- `far`: (6.25, -4.5) px, for windows so wide
    that at the smaller shift most windows over the occluder still find their way back --, 'border' (7.5, 6.25) px towards the
    lower right + occluder (keypoints near that border end outside the frame), 'same', 'unrelated'"""
    h, w = base.shape
    if kind == "same":
        return to_u8(base)
    if kind == "unrelated":
        return to_u8(texture(w, h, seed))
    if kind == "shift":
        dx, dy = (6.25, -4.5) if far else (3.25, -2.5)
        return to_u8(occluded(shifted(base, dx + 0.5 * (seed % 3), dy + 0.75 * (seed % 2)), seed))
    if kind == "border":
        return to_u8(occluded(shifted(base, 7.5, 6.25), seed, 0.1, 0.5))
    raise ValueError(kind)


def thr2_of(thr: float) -> np.float32:
    return np.float32(np.float64(thr) * np.float64(thr))


def composed(p1: oracle.Pyramid, pt: oracle.Pyramid, kps: np.ndarray, opt, thr: float):
    """-> dict(next_xy, status_f, err, back_xy, back_status, status, d2) for one target, all [N]"""
    kps = np.ascontiguousarray(kps, np.float32).reshape(-1, 2)
    n = len(kps)
    q, sf, err = oracle.lk(p1, pt, kps, opt)
    idx = np.nonzero(sf == 1)[0]
    bxy, bst = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
    if len(idx):
        b, sb, _ = oracle.lk(pt, p1, q[idx], opt)
        bxy[idx], bst[idx] = b, sb
    dx = (bxy[:, 0] - kps[:, 0]).astype(np.float32)
    dy = (bxy[:, 1] - kps[:, 1]).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
        keep = (sf == 1) & (bst == 1) & (d2 <= thr2_of(thr))
    return {"next_xy": q, "status_f": sf, "err": err, "back_xy": bxy, "back_status": bst, "status": keep.astype(np.uint8), "d2": d2}


def check_fractions(c: dict, kind: str):
    """the scene must exercise both outcomes: asserted on the ORACLE's result, before anything is compared with it"""
    fwd = int((c["status_f"] == 1).sum())
    kept = int(c["status"].sum())
    if kind == "same":
        assert fwd > 0 and kept == fwd, (kind, fwd, kept)
        assert not c["d2"][c["status_f"] == 1].any()
        return
    assert fwd >= 10, (kind, fwd)
    assert fwd - kept >= 0.1 * fwd, (kind, fwd, kept)
    if kind != "unrelated":
        assert kept >= 0.1 * fwd, (kind, fwd, kept)


def clip(w: int, h: int, n: int, seed: int = 7):
    """n RGB uint8 frames: a texture drifting by (1.25, -0.5) px per frame behind a fixed rectangle whose content changes with
    every frame (nothing tracks into or out of it)"""
    base = texture(w + 64, h + 64, seed)
    frames = []
    for t in range(n):
        g = shifted(base, 1.25 * t, -0.5 * t)[32:32 + h, 32:32 + w]
        g = to_u8(occluded(g, 1000 + seed + t))
        frames.append(np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)))
    return frames
