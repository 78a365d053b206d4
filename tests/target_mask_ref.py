"""CPU reference of target-side masks (include/polychase_hip.h: pc_lk_track_masked), in numpy.  TEST INFRASTRUCTURE ONLY.

  on(x, y)    the mask byte is non-zero
  choke(m, r) C_r(x, y) = 255 when on(x', y') for every pixel OF THE FRAME with |x' - x| <= r and |y' - y| <= r, else 0:
              pixels outside the frame are ignored (= padding with "on"); C_0 is the mask read as on/off
  pixel(q)    ix = (int) fminf(fmaxf(floorf(q.x + 0.5f), 0), w - 1), iy likewise: every operation in float32, an end point
              outside the frame lands on the nearest border pixel, a NaN on 0
  keep        status & (C_r[iy, ix] != 0) for a target with a mask; a target without one keeps its rows

choke() is written as the definition -- an AND over the (2 r + 1)^2 shifted copies of the padded plane -- not as the separable
two-pass form the kernel uses."""
from __future__ import annotations

import numpy as np

MAX_MARGIN = 31


def choke(mask: np.ndarray, r: int) -> np.ndarray:
    if not 0 <= int(r) <= MAX_MARGIN:
        raise ValueError(f"margin {r}, 0..{MAX_MARGIN} allowed")
    on = np.asarray(mask) != 0
    assert on.ndim == 2
    h, w = on.shape
    r = int(r)
    pad = np.ones((h + 2 * r, w + 2 * r), bool)
    pad[r:r + h, r:r + w] = on
    out = np.ones((h, w), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= pad[dy:dy + h, dx:dx + w]
    return out.astype(np.uint8) * 255


def pixel(xy: np.ndarray, w: int, h: int):
    """end points float32 [..., 2] -> (ix, iy) int64 arrays"""
    xy = np.asarray(xy, np.float32)
    half, zero = np.float32(0.5), np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.fmin(np.fmax(np.floor((xy[..., 0] + half).astype(np.float32)), zero), np.float32(w - 1))
        fy = np.fmin(np.fmax(np.floor((xy[..., 1] + half).astype(np.float32)), zero), np.float32(h - 1))
    return fx.astype(np.int64), fy.astype(np.int64)


def keep(xy: np.ndarray, status: np.ndarray, mask: np.ndarray | None, r: int) -> np.ndarray:
    """the status after the test: rows [N] that end in a frame with mask `mask` (None: no mask, every row kept) under margin r"""
    status = np.asarray(status, np.uint8)
    if mask is None:
        return status.copy()
    h, w = np.asarray(mask).shape
    ix, iy = pixel(xy, w, h)
    return (status & (choke(mask, r)[iy, ix] != 0)).astype(np.uint8)
