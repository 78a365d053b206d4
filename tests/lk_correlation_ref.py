"""The minimum-correlation rule of include/polychase_hip.h (pc_lk_track_correlated), restated in numpy.  TEST INFRASTRUCTURE ONLY.

A forward row (keypoint p, end point q, status 1) is judged by the two win x win windows LK itself compared at level 0:
    I = window_values(gray1, win, p.x, p.y)        what the template pass takes at p - half (oracle/pc_oracle.c:567-597)
    J = window_values(grayT, win, q.x, q.y)        what the err pass evaluates at q - half (:729-748), before I is subtracted
both x 32 in 0..8160.  From exact integer sums
    cov = n sum(IJ) - sum(I) sum(J),  vI = n sum(I^2) - sum(I)^2,  vJ = n sum(J^2) - sum(J)^2
the row is kept iff cov > 0 and float64(cov)^2 >= (float64(vI) * float64(vJ)) * float64(thr)^2, every operation rounded on its
own; score = float32(float64(cov) / sqrt(float64(vI) * float64(vJ))), 0 when either variance is 0."""
from __future__ import annotations

import math

import numpy as np

W_BITS = 14


def window_values(gray: np.ndarray, win: int, x, y):
    """int64 (win, win) or None when the window fails OpenCV's bounds test.  gray: uint8 (h, w); (x, y): the window's CENTRE as
    LK holds it (a keypoint, an end point), float32."""
    h, w = gray.shape
    half = np.float32(win - 1) * np.float32(0.5)
    px, py = np.float32(x) - half, np.float32(y) - half
    if not (np.isfinite(px) and np.isfinite(py)):
        return None
    ipx, ipy = int(np.floor(px)), int(np.floor(py))
    if ipx < -win or ipx >= w or ipy < -win or ipy >= h:
        return None
    one, scale = np.float32(1.0), np.float32(1 << W_BITS)
    a, b = px - np.float32(ipx), py - np.float32(ipy)
    iw00 = int(np.rint((one - a) * (one - b) * scale))
    iw01 = int(np.rint(a * (one - b) * scale))
    iw10 = int(np.rint((one - a) * b * scale))
    iw11 = (1 << W_BITS) - iw00 - iw01 - iw10          # may be -1
    pad = win + 1
    plane = np.pad(gray, pad, mode="reflect").astype(np.int64)      # REFLECT_101
    r0, c0 = ipy + pad, ipx + pad
    s = plane[r0:r0 + win + 1, c0:c0 + win + 1]
    v = s[:-1, :-1] * iw00 + s[:-1, 1:] * iw01 + s[1:, :-1] * iw10 + s[1:, 1:] * iw11
    return (v + (1 << (W_BITS - 5 - 1))) >> (W_BITS - 5)            # DESCALE(., 9)


def sums(I: np.ndarray, J: np.ndarray):
    """-> (cov, vI, vJ), Python integers"""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    n = int(I.size)
    sI, sJ = int(I.sum()), int(J.sum())
    sII, sJJ, sIJ = int((I * I).sum()), int((J * J).sum()), int((I * J).sum())
    return n * sIJ - sI * sJ, n * sII - sI * sI, n * sJJ - sJ * sJ


def keep(cov: int, vI: int, vJ: int, thr: float) -> bool:
    t2 = float(np.float64(thr) * np.float64(thr))
    return cov > 0 and float(cov) * float(cov) >= (float(vI) * float(vJ)) * t2


def score(cov: int, vI: int, vJ: int) -> np.float32:
    if vI == 0 or vJ == 0:
        return np.float32(0.0)
    return np.float32(float(cov) / math.sqrt(float(vI) * float(vJ)))


def rows(gray1: np.ndarray, gray_t: np.ndarray, win: int, kps: np.ndarray, next_xy: np.ndarray, status: np.ndarray, thr: float):
    """one target's rows -> (keep uint8 [N], score float32 [N]): keep = status AND the rule (thr 0: status itself); the score is
    0 where status is 0 or a window fails the bounds test"""
    n = len(kps)
    k, sc = np.zeros(n, np.uint8), np.zeros(n, np.float32)
    for i in np.nonzero(np.asarray(status) == 1)[0]:
        I = window_values(gray1, win, kps[i, 0], kps[i, 1])
        J = window_values(gray_t, win, next_xy[i, 0], next_xy[i, 1])
        if I is None or J is None:
            k[i] = 1 if thr == 0 else 0
            continue
        c = sums(I, J)
        k[i] = 1 if thr == 0 or keep(*c, thr) else 0
        sc[i] = score(*c)
    return k, sc
