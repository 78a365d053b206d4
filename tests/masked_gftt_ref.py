"""CPU reference of GoodFeaturesToTrack WITH its mask argument (reference cpp/feature_detection/gftt.cc:38-181), in numpy.
TEST INFRASTRUCTURE ONLY.

The raw response map comes from the oracle (oracle.min_eigen_val / oracle.corner_harris, in the oracle's current emulation
mode); everything behind it is restated here, because oracle/pc_oracle.c's pco_gftt has no mask:
  per grid cell  maxVal = max over the cell's pixels whose mask byte is non-zero (0.0 for a cell with none: what
                 cv::minMaxLoc leaves for an empty mask -- recalled from OpenCV)        gftt.cc:58-63
                 threshold (float)(maxVal * quality_level), THRESH_TOZERO, on EVERY pixel of the cell   gftt.cc:64-66
  3 x 3 dilation over everything                                                                       gftt.cc:69
  candidates     strictly interior, val != 0, val == dilated, mask byte non-zero                        gftt.cc:76-86
  sort           value descending, then address descending                                             gftt.cc:7-12, :98
  greedy loop    3 x 3 cells of cvRound(min_distance), float32 dx * dx + dy * dy against the double min_distance^2;
                 max_corners                                                                           gftt.cc:100-181
With mask=None (or all non-zero) this is oracle.gftt, keypoint for keypoint (tests/test_detection_mask_cpu.py).
"""
from __future__ import annotations

import numpy as np

import oracle


def response(gray: np.ndarray, opt) -> np.ndarray:
    if opt.use_harris:
        return oracle.corner_harris(gray, opt.block_size, opt.gradient_size, opt.harris_k)
    return oracle.min_eigen_val(gray, opt.block_size, opt.gradient_size)


def candidates(eig: np.ndarray, opt, mask: np.ndarray | None):
    """-> (values float32 [n], linear indices int64 [n]) in processing order (value desc, address desc)"""
    h, w = eig.shape
    on = np.ones((h, w), bool) if mask is None else (np.asarray(mask) != 0)
    assert on.shape == (h, w)
    rows, cols = max(1, opt.grid_rows), max(1, opt.grid_cols)
    bh, bw = (h + rows - 1) // rows, (w + cols - 1) // cols
    thr_map = np.zeros((h, w), np.float32)
    for gy in range(rows):
        for gx in range(cols):
            y0, x0 = gy * bh, gx * bw
            y1, x1 = min(y0 + bh, h), min(x0 + bw, w)
            if y0 >= y1 or x0 >= x1:
                continue
            cell, cell_on = eig[y0:y1, x0:x1], on[y0:y1, x0:x1]
            max_val = float(cell[cell_on].max()) if cell_on.any() else 0.0
            thr_map[y0:y1, x0:x1] = np.float32(max_val * opt.quality_level)     # double product, rounded to float
    t = np.where(eig > thr_map, eig, np.float32(0)).astype(np.float32)
    pad = np.full((h + 2, w + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = t
    dil = t.copy()
    for j in range(3):
        for i in range(3):
            np.maximum(dil, pad[j:j + h, i:i + w], out=dil)
    interior = np.zeros((h, w), bool)
    interior[1:h - 1, 1:w - 1] = True
    ys, xs = np.nonzero(interior & (t != 0) & (t == dil) & on)
    vals = t[ys, xs]
    idx = ys.astype(np.int64) * w + xs
    order = np.lexsort((-idx, -vals.astype(np.float64)))    # primary: value descending; ties: address descending
    return vals[order], idx[order]


def suppress(idx: np.ndarray, w: int, h: int, opt) -> np.ndarray:
    ys, xs = idx // w, idx % w
    if not opt.min_distance >= 1:
        n = len(idx) if opt.max_corners <= 0 else min(len(idx), opt.max_corners)
        return np.stack([xs[:n], ys[:n]], 1).astype(np.float32).reshape(-1, 2)
    cell = int(np.rint(opt.min_distance))          # cvRound: half to even, like lrint
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    r2 = float(opt.min_distance) * float(opt.min_distance)
    grid: dict[int, list] = {}
    out = []
    for x, y in zip(xs.tolist(), ys.tolist()):
        xc, yc = x // cell, y // cell
        good = True
        for yy in range(max(yc - 1, 0), min(yc + 1, gh - 1) + 1):
            for xx in range(max(xc - 1, 0), min(xc + 1, gw - 1) + 1):
                for (ax, ay) in grid.get(yy * gw + xx, ()):
                    dx, dy = np.float32(x) - np.float32(ax), np.float32(y) - np.float32(ay)
                    if float(np.float32(np.float32(dx * dx) + np.float32(dy * dy))) < r2:
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid.setdefault(yc * gw + xc, []).append((x, y))
            out.append((x, y))
            if opt.max_corners > 0 and len(out) == opt.max_corners:
                break
    return np.array(out, np.float32).reshape(-1, 2)


def gftt(gray: np.ndarray, opt=None, mask: np.ndarray | None = None):
    """-> (keypoints float32 [n, 2] in acceptance order, raw response map, candidate count)"""
    opt = opt or oracle.gftt_options()
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    eig = response(gray, opt)
    vals, idx = candidates(eig, opt, mask)
    return suppress(idx, w, h, opt), eig, len(idx)


def post_filtered(gray: np.ndarray, opt, mask: np.ndarray) -> np.ndarray:
    """what a mask applied AFTER an unmasked detection would keep (the implementation the feature must not be)"""
    kps = gftt(gray, opt, None)[0]
    keep = np.asarray(mask)[kps[:, 1].astype(int), kps[:, 0].astype(int)] != 0
    return kps[keep]


# the option sets and masks shared by the CPU and the GPU tests
OPTION_SETS = {
    "default": {},
    "nodist": dict(min_distance=0.0),
    "harris": dict(use_harris=1),
    "block5_sobel5": dict(block_size=5, gradient_size=5),
    "grid3x5_dist9": dict(grid_rows=3, grid_cols=5, min_distance=9.0),
    "max50": dict(max_corners=50),
}


def test_image(w: int, h: int, seed: int = 7) -> np.ndarray:
    """weak smoothed noise plus strong squares, one of them under the disc of mask_column_and_disc: masking it out lowers
    the threshold of its grid cell, so weak corners appear that an unmasked detection never reports"""
    rng = np.random.default_rng(seed + 131 * w + h)
    a = rng.integers(0, 256, (h + 4, w + 4)).astype(np.float32)
    a = (a[:-4, :-4] + a[2:-2, 2:-2] + a[4:, 4:] + a[:-4, 4:] + a[4:, :-4]) / 5.0
    img = (96.0 + (a - 128.0) * 0.25).astype(np.uint8)
    for k, (fx, fy) in enumerate([(0.62, 0.45), (0.12, 0.2), (0.85, 0.8), (0.4, 0.85), (0.3, 0.3), (0.9, 0.15)]):
        x, y = int(fx * w) - 3, int(fy * h) - 3
        img[y:y + 6, x:x + 7] = 255 if k % 2 == 0 else 0
    return img


def mask_column_and_disc(w: int, h: int, cols: int = 4, seed: int = 3) -> np.ndarray:
    """the left column of grid cells fully off, a disc hole, the "on" bytes drawn from {1, 128, 255}"""
    rng = np.random.default_rng(seed)
    m = rng.choice(np.array([1, 128, 255], np.uint8), size=(h, w))
    m[:, :(w + cols - 1) // cols] = 0
    yy, xx = np.mgrid[0:h, 0:w]
    m[(xx - 0.62 * w) ** 2 + (yy - 0.45 * h) ** 2 < max(6.0, 0.15 * min(w, h)) ** 2] = 0   # covers test_image's first square
    return np.ascontiguousarray(m)


def mask_speckle(w: int, h: int, seed: int = 5) -> np.ndarray:
    return (np.random.default_rng(seed).random((h, w)) < 0.5).astype(np.uint8) * 255


def mask_ring(w: int, h: int) -> np.ndarray:
    m = np.zeros((h, w), np.uint8)
    m[0, :] = m[-1, :] = 255
    m[:, 0] = m[:, -1] = 255
    return m
