"""CPU: what the scenes of tests/lk_subpixel_scene.py must exercise, asserted on the keypoints and on the ORACLE's results alone
-- before test_lk_subpixel_gpu.py and _lk_plain_check.py compare a kernel with them (the precedent: fb_scene.check_fractions)."""
import numpy as np
import pytest

import lk_subpixel_scene as scene
import oracle

ARITH = ("canonical", "lk_x86_order")


@pytest.mark.parametrize("win", scene.WINDOWS)
def test_keypoint_classes_are_what_they_are_built_for(win):
    """B: w11 == -1 at level 0; C: three exact .5 ties; D: on both sides of the bounds test; E: out of range.  In float32 numpy
    in the oracle's expression order."""
    g1, targets, kps = scene.scene(win)
    assert g1.shape == (scene.H, scene.W) and len(targets) == (1, 3, 8)[win % 3] and len(kps) == 471
    assert [len(range(*s.indices(len(kps)))) for s in scene.CLASSES.values()] == [97, 256, 64, 48, 6]
    scene.check_classes(win)
    # a frame with three equal channels converts to itself: what the analyzer path is fed
    assert np.array_equal(oracle.rgb2gray(scene.rgb(g1)), g1)


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("win", scene.WINDOWS)
def test_oracle_results_show_every_outcome(win, arith):
    exp = scene.expected(win, arith)
    kps = scene.scene(win)[2]
    out = scene.template_out_of_range(kps, win)
    for t, (xy, st, err) in enumerate(exp):
        d = st[scene.CLASSES["D"]]
        assert (d == 1).sum() >= 3 and (d == 0).sum() >= 3, (win, arith, t, int((d == 1).sum()), "of 48 ring points tracked")
        e = scene.CLASSES["E"]
        assert not st[e].any() and not err[e].view(np.uint32).any(), (win, arith, t)
        assert not st[out].any() and not err[st == 0].view(np.uint32).any(), (win, arith, t)
        if scene.target_kinds(win)[t] == "same":
            # an unchanged target leaves class B where it started, bit for bit: the first iteration and the patch error at level
            # 0 evaluate the SEARCHED side with w11 == -1 too (a 1e-9 event per iteration otherwise)
            b = scene.CLASSES["B"]
            assert st[b].all() and np.array_equal(scene.bits(xy[b]), scene.bits(kps[b])), (win, arith, t)
    # the plain shifted target: the general points follow the known flow
    xy, st, err = exp[0]
    a = scene.CLASSES["A"]
    m = st[a] == 1
    assert m.sum() >= 0.8 * scene.N_A, (win, arith, int(m.sum()))
    gt = kps[a] + np.array(scene.SHIFT, np.float32)
    med = float(np.median(np.abs(xy[a][m] - gt[m])))
    print("window", win, arith, "A tracked", int(m.sum()), "median error", round(med, 4), "ring tracked per target",
          [int((s[scene.CLASSES["D"]] == 1).sum()) for _, s, _ in exp])
    assert med < 0.1, (win, arith, med)


def test_comparison_names_the_class_of_a_planted_difference():
    """the rule the GPU tests apply (scene.mismatch): one flipped bit in a tracked row is reported with its class; rows the oracle
    did not track are held to status 0 and err 0 only"""
    win = 10
    exp = scene.expected(win, "canonical")
    good = tuple(np.stack([e[k] for e in exp]) for k in range(3))
    assert scene.mismatch(win, good, exp) == ""
    t = len(exp) - 1
    for name in "ABCD":
        s = scene.CLASSES[name]
        i = s.start + int(np.nonzero(exp[t][1][s] == 1)[0][-1])
        for k, what in ((0, "next_xy"), (2, "err")):
            bad = [a.copy() for a in good]
            bad[k].view(np.uint32)[t, i] ^= 1
            why = scene.mismatch(win, bad, exp)
            assert ("target %d" % t) in why and what in why and ("%s[%d]" % (name, i - s.start)) in why, why
        bad = [a.copy() for a in good]
        bad[1][t, i] = 0
        assert "status differs at %s[" % name in scene.mismatch(win, bad, exp)
    e0 = scene.CLASSES["E"].start
    bad = [a.copy() for a in good]
    bad[0][0, e0] += 1.0                      # not tracked: next_xy is free
    assert scene.mismatch(win, bad, exp) == ""
    bad[2][0, e0] = 1e-30                     # ... err is not
    assert "err differs at E[0]" in scene.mismatch(win, bad, exp)
    rows = [(np.nonzero(st == 1)[0].astype(np.uint32), xy[st == 1], err[st == 1]) for xy, st, err in exp]
    assert scene.filtered_mismatch(rows, good) == ""
    rows[t] = (rows[t][0][::-1].copy(), rows[t][1][::-1].copy(), rows[t][2][::-1].copy())
    assert scene.filtered_mismatch(rows, good) != ""


def test_expected_arrays_are_shared_and_read_only():
    exp = scene.expected(7, "canonical")
    assert exp is scene.expected(7, "canonical")
    for arrays in exp:
        for a in arrays:
            assert not a.flags.writeable
    assert not scene.scene(7)[2].flags.writeable
