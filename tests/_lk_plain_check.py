#!/usr/bin/env python3
"""Helper of tests/test_lk_plain_gpu.py: the plain forward LK kernel (lk_plain_kernel, csrc/hip/kernels_lk.hip), which only runs
under POLYCHASE_LK_VARIANT=1 -- a switch the library reads once per process, hence this process -- against the CPU oracle, bit
for bit, in both arithmetic orders.  All cases run here, one after the other; one line per case: "PASS <case> <arith>" or
"FAIL <case> <arith> <what differs>".

The expected arrays are functions of this module (computed on the CPU, cached, never modified), so that the test file can hold
the product kernels of the default variant against the very same arrays."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fb_scene  # noqa: E402
import lk_subpixel_scene as subpixel  # noqa: E402
import oracle  # noqa: E402
from polychase_amd import hip, synth  # noqa: E402
from test_lk_fb_gpu import CASES, _scene  # noqa: E402  (the six scenes of the forward-backward check: not copied)

ARITH = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL), "lk_x86_order": (hip.ARITH_LK_X86_ORDER, oracle.EMU_LK_SIMD)}

# (window, max_level, targets) on the checkerboard: the content on which the two summation orders give different bits.  The vector
# blocks of the x86 order cover 0 + 7, 8 + 0, 8 + 1, 8 + 2, 8 + 7, 16 + 0, 16 + 1, 24 + 0 and 24 + 7 columns.
BOARD_CASES = [(7, 2, 2), (8, 3, 5), (9, 2, 4), (10, 3, 8), (15, 3, 8), (16, 2, 3), (17, 2, 2), (24, 2, 2), (31, 2, 4)]
BOARD_W, BOARD_H = 320, 240
LK4_CROSS_CHECKED = [c for c in BOARD_CASES if c[0] in (17, 24, 31)]   # windows no other kernel cross-checked before
# (scene, target) whose forward pass tracks EVERY keypoint on the oracle (422 of 422 and 428 of 428 in both orders): these 'shift'
# targets lose their points only in the backward pass, so they cannot show both forward outcomes
ALL_TRACKED = {("160x120_w15_l2", 5), ("160x120_w31_l2", 0)}
# windows of tests/lk_subpixel_scene.py: keypoints off the integer grid (w11 == -1, rounding ties) and out of the frame; the product
# kernels meet the same expected arrays in test_lk_subpixel_gpu.py
SUBPIXEL_WINDOWS = (3, 7, 10, 16, 31)


def _frozen(per_target):
    for arrays in per_target:
        for a in arrays:
            a.setflags(write=False)
    return per_target


def _oracle_lk(g1, targets, kps, win, ml, arith):
    """[(next_xy, status, err)] per target: oracle.lk, the forward half of fb_scene.composed"""
    opt = oracle.flow_options(window_size=win, max_level=ml)
    with oracle.emulation(ARITH[arith][1]):
        p1 = oracle.Pyramid(g1, win, ml)
        return _frozen([oracle.lk(p1, oracle.Pyramid(t, win, ml), kps, opt) for t in targets])


@functools.lru_cache(maxsize=None)
def scene_expected(case, arith):
    w, h, win, ml, kinds = CASES[case]
    g1, targets, kps = _scene(case)
    return _oracle_lk(g1, targets, kps, win, ml, arith)


def counts_scene(n):
    """n supplied keypoints at fractional positions within a window of each border, a flat target among the three: the scene of
    test_lk_fb_gpu.py: test_keypoint_counts_border_positions_and_a_target_without_survivors"""
    w, h, win, ml = 96, 80, 7, 2
    base = fb_scene.texture(w, h, 5)
    tg = [fb_scene.target(base, "shift", 3), np.full((h, w), 90, np.uint8), fb_scene.target(base, "border", 4)]
    pos = np.array([[1.3, 2.6], [w - 2.25, 3.5], [4.75, h - 1.5], [w - 6.5, h - 3.125], [0.0, 0.0], [w - 1.0, h - 1.0],
                    [40.5, 0.25], [0.75, 41.5], [w - 1.5, 30.25], [50.125, h - 2.75], [30.3, 30.7], [60.6, 50.2], [6.9, 6.1]], np.float32)
    return (w, h, win, ml), fb_scene.to_u8(base), tg, pos[:n]


@functools.lru_cache(maxsize=None)
def board_scene():
    frames = [oracle.rgb2gray(f) for f in synth.checkerboard_clip(16, w=BOARD_W, h=BOARD_H)]
    kps = oracle.gftt(frames[6])
    assert len(kps) == 80, len(kps)
    return frames[6], frames[7:], kps


@functools.lru_cache(maxsize=None)
def board_expected(case, arith):
    win, ml, nt = case
    g1, later, kps = board_scene()
    return _oracle_lk(g1, later[:nt], kps, win, ml, arith)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def orders_differ(case):
    """tracked vectors of a checkerboard case whose bits differ between the two orders (on the oracle alone)"""
    n = 0
    for (xa, sa, _), (xb, sb, _) in zip(board_expected(case, "canonical"), board_expected(case, "lk_x86_order")):
        both = (sa == 1) & (sb == 1)
        n += int((bits(xa)[both] != bits(xb)[both]).any(axis=1).sum())
    return n


def gpu_lk(ctx, size, g1, targets, kps):
    w, h, win, ml = size
    fr = []
    for g in [g1] + list(targets):
        f = hip.Frame(ctx, w, h, win, ml)
        f.set_gray(g)
        fr.append(f)
    fr[0].set_keypoints(kps)
    out = hip.lk_track(ctx, fr[0], fr[1:], hip.flow_options(window_size=win, max_level=ml))
    for f in fr:
        f.close()
    return out


def mismatch(got, expected):
    """'' when next_xy, status and err of every target equal the oracle's bit for bit, else what differs first"""
    xy, st, err = got
    if xy.shape[0] != len(expected):
        return f"{xy.shape[0]} targets, expected {len(expected)}"
    for t, (exy, est, eerr) in enumerate(expected):
        for name, a, b in (("status", st[t], est), ("next_xy", bits(xy[t]), bits(exy)), ("err", bits(err[t]), bits(eerr))):
            if a.shape != b.shape or not np.array_equal(a, b):
                rows = np.nonzero(np.atleast_2d((a != b).T).any(axis=0))[0] if a.shape == b.shape else []
                return f"target {t}: {name} differs in {len(rows)} of {len(b)} rows (first {list(rows[:4])})"
    return ""


def board_gpu_mismatch(ctx, case, arith):
    win, ml, nt = case
    g1, later, kps = board_scene()
    return mismatch(gpu_lk(ctx, (BOARD_W, BOARD_H, win, ml), g1, later[:nt], kps), board_expected(case, arith))


def board_name(case):
    return "board_w%d_l%d_t%d" % case


def subpixel_name(win):
    return "subpixel_w%d" % win


def subpixel_gpu_mismatch(ctx, win, arith):
    g1, targets, kps = subpixel.scene(win)
    got = gpu_lk(ctx, (subpixel.W, subpixel.H, win, subpixel.MAX_LEVEL), g1, targets, kps)
    exp = subpixel.expected(win, arith)
    # first by class and keypoint (the product kernels' rule: the tracked rows), then every row like the cases above
    return subpixel.mismatch(win, got, exp) or mismatch(got, exp)


def case_names():
    return sorted(CASES) + ["counts_5", "counts_13"] + [board_name(c) for c in BOARD_CASES] + [subpixel_name(w) for w in SUBPIXEL_WINDOWS]


def main():
    assert os.environ.get("POLYCHASE_LK_VARIANT") == "1", "this helper is about the kernel behind POLYCHASE_LK_VARIANT=1"
    # what the scenes must exercise, asserted on the ORACLE's results before anything is compared with them
    for case in sorted(CASES):
        for arith in sorted(ARITH):
            for t, (kind, (_, st, _)) in enumerate(zip(CASES[case][4], scene_expected(case, arith))):
                one_outcome = kind == "same" or (case, t) in ALL_TRACKED
                assert (st == 1).any() and (st == 0).any() != one_outcome, (case, arith, t, kind, int(st.sum()), len(st))
    for case in BOARD_CASES:
        assert orders_differ(case) >= 1, (case, "the two summation orders agree on every vector")
    for win in SUBPIXEL_WINDOWS:
        subpixel.check_classes(win)

    for arith in sorted(ARITH):
        ctx = hip.Context(0)
        ctx.set_arithmetic(ARITH[arith][0])

        def report(name, why):
            print(("FAIL %s %s %s" % (name, arith, why)) if why else ("PASS %s %s" % (name, arith)), flush=True)

        for case in sorted(CASES):
            w, h, win, ml, kinds = CASES[case]
            g1, targets, kps = _scene(case)
            report(case, mismatch(gpu_lk(ctx, (w, h, win, ml), g1, targets, kps), scene_expected(case, arith)))
        for n in (5, 13):   # the last workgroup is partly empty
            size, g1, targets, kps = counts_scene(n)
            report("counts_%d" % n, mismatch(gpu_lk(ctx, size, g1, targets, kps), _oracle_lk(g1, targets, kps, size[2], size[3], arith)))
        for case in BOARD_CASES:
            report(board_name(case), board_gpu_mismatch(ctx, case, arith))
        for win in SUBPIXEL_WINDOWS:
            report(subpixel_name(win), subpixel_gpu_mismatch(ctx, win, arith))
        ctx.close()


if __name__ == "__main__":
    main()
