"""Scenes for the parity of the forward LK kernels OFF THE INTEGER GRID (tests/test_lk_subpixel_cpu.py, test_lk_subpixel_gpu.py
and the subpixel_* cases of _lk_plain_check.py).  TEST INFRASTRUCTURE ONLY: numpy, fb_scene and the oracle, nothing from the GPU.

Detected (GFTT) keypoints are integers, so on the template ("I") side of pco_lk the bilinear fractions are dyadic (0 or 0.5 at
level 0), every weight product is exact, cvRound never rounds and w11 = 2^14 - w00 - w01 - w10 is never -1.  One scene per
window 3 .. 31 feeds the C ABI what it also accepts: 112 x 96 images, max_level 2 (the pyramid ends early at wide windows),
(1, 3, 8)[win % 3] targets and ONE float32 keypoint array of 471 points (odd: the last two-keypoint wavefront has an empty
half), the concatenation of five classes (CLASSES):

  A  97 points uniform in [0, w-1] x [0, h-1]
  B  256 points with w11 == -1 on the I side at level 0: a = ka / 2^18, b = kb / 2^18 with ka, kb in 9 .. 11 (10 where the
     coordinate is >= 64 and float32 steps by 2^-17), so that a * 2^14 and b * 2^14 lie in (0.5, 1) and their sum below 1.5:
     w01 = w10 = 1, w00 = 2^14 - 1; cells at least `win` from the border.  On an unchanged ('same') target these points stay
     where they are bit for bit, so there the searched side sees w11 == -1 as well (windows with 3 or 8 targets)
  C  64 points with a = 0.5, b = odd / 2^14: the three products behind w00, w01 and w10 are exact .5 ties (lrintf rounds them to
     even; rounding half up gives other weights)
  D  48 points uniform in the ring [-(win+3), w-1+win+3] x [-(win+3), h-1+win+3] whose window does not lie wholly inside the
     frame: in the REFLECT_101 / zero Scharr padding, and just beyond it (status 0)
  E  6 far points (|coordinate| <= 1e6): status 0 and err 0 at every window

B and C are asserted here in float32 numpy, in the oracle's own expression order (level0_weights), before anything is tracked.

Discrimination, measured once on the CPU with two mutated copies of oracle/pc_oracle.c (not kept): keypoints whose tracked rows
(next_xy, err, status on any target, canonical order) differ from the real oracle's.
  * I-side iw11 clamped at >= 0, class B, of 256, windows 3 .. 31:
      16 23 29 45 42 76 91 110 144 136 156 185 174 131 201 227 244 231 232 250 229 256 256 255 256 256 256 256 256
  * I-side cvRound as floorf(0.5f + x), class C, of 64, windows 3 .. 31:
      47 63 62 64 63 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64 64
The x86 order gives the same counts.  Neither mutant touches another class, except that the rounding mutant moves 0 .. 2 of the
97 points of class A at a few windows (a float32 fraction now and then lands on a tie by itself); integer keypoints see
neither mutant.  The oracle, not OpenCV itself, is the reference for these inputs: the
committed OpenCV golden (tests/golden) tracks integer keypoints only."""
from __future__ import annotations

import functools

import numpy as np

import fb_scene
import oracle

W, H, MAX_LEVEL = 112, 96, 2
WINDOWS = tuple(range(3, 32))
SHIFT = (2.3, -1.7)
KINDS = ("shifted", "border", "same")
# arithmetic order by name -> the oracle's emulation flags: the two of _lk_plain_check.ARITH, and the library's default
EMU = {"canonical": oracle.EMU_CANONICAL, "lk_x86_order": oracle.EMU_LK_SIMD, "opencv_x86": oracle.EMU_OPENCV_X86}
N_A, N_B, N_C, N_D = 97, 256, 64, 48
FAR = ((-1e6, 40.3), (50.7, 1e6), (1e6, 1e6), (-300.5, -200.25), (3 * W + 0.4, 10.1), (20.2, -2 * H - 0.6))
CLASSES = {}
_o = 0
for _name, _n in (("A", N_A), ("B", N_B), ("C", N_C), ("D", N_D), ("E", len(FAR))):
    CLASSES[_name] = slice(_o, _o + _n)
    _o += _n
N_POINTS = _o
assert N_POINTS == 471
W_BITS = 14
# A seed under which the ring (class D) shows at least 3 points of either status on every target at every window
# (test_lk_subpixel_cpu.py).  A 3-px window partly in the padding rarely tracks -- one or two of 48 under most seeds --, and a
# seed that misses is replaced, the bound stays.
KEYPOINT_SEED = 100007


def n_targets(win: int) -> int:
    return (1, 3, 8)[win % 3]


def target_kinds(win: int):
    return [KINDS[i % 3] for i in range(n_targets(win))]


def class_of(i: int) -> str:
    """'B[17]' for keypoint index i"""
    for name, s in CLASSES.items():
        if s.start <= i < s.stop:
            return "%s[%d]" % (name, i - s.start)
    raise IndexError(i)


def _frac_half(win: int) -> np.float32:
    return np.float32(0.5 if win % 2 == 0 else 0.0)   # the fractional part of half_win = (win - 1) / 2


def _cells(rng, n, win):
    """integer cells whose window lies inside the frame with `win` to spare"""
    return np.stack([rng.integers(win, W - win, n), rng.integers(win, H - win, n)], axis=1).astype(np.float32)


def _keypoints(win: int) -> np.ndarray:
    rng = np.random.default_rng(KEYPOINT_SEED + win)
    f32 = np.float32
    a_pts = (rng.uniform(0.0, 1.0, (N_A, 2)) * np.array([W - 1, H - 1])).astype(f32)

    cell = _cells(rng, N_B, win)
    k = rng.integers(9, 12, (N_B, 2)).astype(f32)
    k[cell >= 64] = 10.0                                       # float32 steps by 2^-17 there: 10 * 2^-18 is five of them
    b_pts = cell + _frac_half(win) + k * f32(2.0 ** -18)       # exact: every term is a multiple of the sum's ulp

    cell = _cells(rng, N_C, win)
    odd = (2 * rng.integers(0, 1 << (W_BITS - 1), N_C) + 1).astype(f32)
    c_pts = cell + _frac_half(win)
    c_pts[:, 0] += f32(0.5)
    c_pts[:, 1] += odd * f32(2.0 ** -W_BITS)

    d_pts = np.zeros((0, 2), f32)
    m = win + 3
    while len(d_pts) < N_D:
        cand = (rng.uniform(0.0, 1.0, (N_D, 2)) * np.array([W - 1 + 2 * m, H - 1 + 2 * m]) - m).astype(f32)
        ipx, ipy = level0_weights(cand, win)[:2]
        inside = (ipx >= 0) & (ipx + win <= W - 1) & (ipy >= 0) & (ipy + win <= H - 1)   # taps ipx .. ipx + win
        d_pts = np.concatenate([d_pts, cand[~inside]])[:N_D]

    kps = np.concatenate([a_pts, b_pts.astype(f32), c_pts.astype(f32), d_pts, np.array(FAR, f32)])
    assert kps.dtype == np.float32 and kps.shape == (N_POINTS, 2) and np.isfinite(kps).all() and np.abs(kps).max() <= 1e6
    return kps


def level0_weights(kps: np.ndarray, win: int):
    """-> ipx, ipy, a, b, (w00, w01, w10, w11), (p00, p01, p10): the level-0 template side of pco_lk (oracle/pc_oracle.c:
    lk_range) in float32 numpy, every operation rounded separately and in the oracle's order; p.. are the unrounded products"""
    f32 = np.float32
    kps = np.asarray(kps, f32)
    half_win = f32(win - 1) * f32(0.5)
    px, py = kps[:, 0] * f32(1.0) - half_win, kps[:, 1] * f32(1.0) - half_win
    fx, fy = np.floor(px), np.floor(py)
    a, b = px - fx, py - fy
    assert a.dtype == f32 and b.dtype == f32
    one, s = f32(1.0), f32(1 << W_BITS)
    p00 = (one - a) * (one - b) * s
    p01 = a * (one - b) * s
    p10 = (one - a) * b * s
    assert p00.dtype == f32
    w00, w01, w10 = (np.rint(p).astype(np.int64) for p in (p00, p01, p10))   # lrintf: to nearest, ties to even
    w11 = (1 << W_BITS) - w00 - w01 - w10
    return fx.astype(np.int64), fy.astype(np.int64), a, b, (w00, w01, w10, w11), (p00, p01, p10)


def template_out_of_range(kps: np.ndarray, win: int) -> np.ndarray:
    """the level-0 template window fails pco_lk's bounds test: status 0 and err 0 whatever the target"""
    ipx, ipy = level0_weights(kps, win)[:2]
    return (ipx < -win) | (ipx >= W) | (ipy < -win) | (ipy >= H)


def check_classes(win: int):
    """what classes B, C and E are built for, asserted on the keypoints themselves"""
    kps = scene(win)[2]
    ipx, ipy, a, b, (w00, w01, w10, w11), _ = level0_weights(kps[CLASSES["B"]], win)
    s = np.float32(1 << W_BITS)
    assert ((a * s > 0.5) & (a * s < 1) & (b * s > 0.5) & (b * s < 1) & (a * s + b * s < 1.5)).all(), win
    assert (w11 == -1).all() and (w01 == 1).all() and (w10 == 1).all() and (w00 == (1 << W_BITS) - 1).all(), win
    cell = np.floor(kps[CLASSES["B"]])
    assert (cell >= win).all() and (cell[:, 0] <= W - 1 - win).all() and (cell[:, 1] <= H - 1 - win).all(), win
    assert (ipx >= 0).all() and (ipx + win <= W - 1).all() and (ipy >= 0).all() and (ipy + win <= H - 1).all(), win
    _, _, a, b, (w00, w01, w10, w11), prods = level0_weights(kps[CLASSES["C"]], win)
    assert (a == 0.5).all() and ((b * s) % 2 == 1).all(), win
    for p in prods:
        assert (p - np.floor(p) == 0.5).all(), win
    assert (w11 >= 0).all()
    assert template_out_of_range(kps[CLASSES["E"]], win).all(), win
    d = template_out_of_range(kps[CLASSES["D"]], win)
    assert d.any() and not d.all(), (win, "the ring must reach into the padding and beyond it")
    assert not template_out_of_range(kps[:CLASSES["D"].start], win).any()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def scene(win: int):
    """-> gray frame 1, [gray targets], keypoints [471, 2] float32: shared, read-only"""
    base = fb_scene.texture(W, H, 300 + win, 3)
    targets = []
    for i, kind in enumerate(target_kinds(win)):
        seed = 500 + 13 * win + i
        if kind == "shifted":   # the first one plain (the known flow of test_lk_subpixel_cpu.py), repeats with an occluder
            img = fb_scene.shifted(base, *SHIFT)
            targets.append(fb_scene.to_u8(img if i < 3 else fb_scene.occluded(img, seed)))
        else:
            targets.append(fb_scene.target(base, kind, seed))
    targets = [np.ascontiguousarray(t) for t in targets]   # a shifted image comes out of fancy indexing column-major
    g1, kps = np.ascontiguousarray(fb_scene.to_u8(base)), _keypoints(win)
    _frozen(g1, kps, *targets)
    return g1, targets, kps


def rgb(gray: np.ndarray) -> np.ndarray:
    """the gray image as the RGB frame the analyzer takes: rgb2gray gives it back"""
    return np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))


@functools.lru_cache(maxsize=None)
def expected(win: int, arith: str):
    """[(next_xy, status, err)] per target from oracle.lk under EMU[arith]: computed once, shared, read-only"""
    g1, targets, kps = scene(win)
    opt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    with oracle.emulation(EMU[arith]):
        p1 = oracle.Pyramid(g1, win, MAX_LEVEL)
        return [_frozen(*oracle.lk(p1, oracle.Pyramid(t, win, MAX_LEVEL), kps, opt)) for t in targets]


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def mismatch(win: int, got, exp) -> str:
    """'' when (next_xy [T,N,2], status [T,N], err [T,N]) agree with expected(win, .): status everywhere, next_xy and err bit
    for bit where the oracle's status is 1, err 0 where the status is 0 (class E, the ring's far part); else the first
    differing keypoint, named by its class"""
    xy, st, err = got
    kps = scene(win)[2]
    if xy.shape != (len(exp), N_POINTS, 2) or st.shape != (len(exp), N_POINTS) or err.shape != st.shape:
        return "shapes %s %s %s for %d targets" % (xy.shape, st.shape, err.shape, len(exp))
    for t, (exy, est, eerr) in enumerate(exp):
        ok = est == 1
        bad = {"status": st[t] != est,
               "next_xy": ok & (bits(xy[t]) != bits(exy)).any(axis=1),
               "err": (ok & (bits(err[t]) != bits(eerr))) | (~ok & (bits(err[t]) != 0))}
        for what, rows in bad.items():
            if rows.any():
                i = int(np.nonzero(rows)[0][0])
                per_class = {n: int(rows[s].sum()) for n, s in CLASSES.items() if rows[s].any()}
                return ("target %d (%s): %s differs at %s = keypoint %d (%r, %r): got %r %d %r, oracle %r %d %r; differing rows per class %s"
                        % (t, target_kinds(win)[t], what, class_of(i), i, float(kps[i, 0]), float(kps[i, 1]), xy[t, i].tolist(), int(st[t, i]),
                           float(err[t, i]), exy[i].tolist(), int(est[i]), float(eerr[i]), per_class))
    return ""


def filtered_mismatch(rows, raw) -> str:
    """'' when the per-target (indices, xy, err) rows are the raw arrays filtered on status == 1: ascending indices, same bits"""
    xy, st, err = raw
    if len(rows) != len(st):
        return "%d targets, expected %d" % (len(rows), len(st))
    for t, (idx, rxy, rerr) in enumerate(rows):
        keep = np.nonzero(st[t] == 1)[0].astype(np.uint32)
        if not np.array_equal(idx, keep):
            return "target %d: %d rows, expected %d (or other indices)" % (t, len(idx), len(keep))
        if not np.array_equal(bits(rxy), bits(xy[t][keep])) or not np.array_equal(bits(rerr), bits(err[t][keep])):
            i = int(keep[np.nonzero((bits(rxy) != bits(xy[t][keep])).any(axis=1) | (bits(rerr) != bits(err[t][keep])))[0][0]])
            return "target %d: the row of %s = keypoint %d differs" % (t, class_of(i), i)
    return ""
