"""GPU: affine refinement of the LK flow rows at stage and analyzer level (kernels_lk_affine.hip through pc_lk_track_affine and
pc_analyzer_set_affine_refinement) against the numpy restatement of the rule (tests/lk_affine_ref.py) applied to the oracle's
forward rows, bit for bit, in both arithmetic modes.  The scenes are tests/lk_affine_scene.py's 96 x 80 gray frames and 204
keypoints; the reference of a (window, mode) is computed once for the eight targets and shared."""
import numpy as np
import pytest

import fb_scene
import lk_affine_ref as ref
import lk_affine_scene as scene
import lk_correlation_ref as corr_ref
import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ARITH = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL), "opencv_x86": (hip.ARITH_OPENCV_X86, oracle.EMU_OPENCV_X86)}
MAX_LEVEL = scene.MAX_LEVEL
NAMES = ("next_xy", "status", "err", "back_xy", "back_status", "affine_m", "affine_state")


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_arithmetic(hip.ARITH_CANONICAL)
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _frames(ctx, win, grays, kps):
    fr = []
    for g in grays:
        f = hip.Frame(ctx, scene.W, scene.H, win, MAX_LEVEL)
        f.set_gray(np.array(g))
        fr.append(f)
    fr[0].set_keypoints(np.array(kps, np.float32).reshape(-1, 2))
    return fr


def _close(fr):
    for f in fr:
        f.close()


def _assert_same(got, want, name, what):
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    d = _bits(got) != _bits(want)
    bad = np.nonzero(d.reshape(len(want), -1).any(axis=1))[0] if len(want) else []
    assert not len(bad), (what, name, "rows", bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())


# ---- 1. bit parity of the stage call ----
@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("n_targets", [1, 3, 8])
@pytest.mark.parametrize("win", [3, 10, 21, 31])
def test_stage_call_matches_the_reference_bit_for_bit(ctx, win, n_targets, arith):
    kps, forward, refined = scene.reference(win, scene.MIX8, ARITH[arith][1])
    st = np.stack([r[4] for r in refined[:n_targets]])
    # asserted on the REFERENCE, before anything is compared with it
    assert (st == ref.ACCEPTED).any() and (st == ref.NOT_RUN).any() and ((st == ref.UNCHANGED).any() or n_targets == 1)
    ctx.set_arithmetic(ARITH[arith][0])
    fr = _frames(ctx, win, [scene.frame1()] + scene.targets(win, n_targets), kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    got = hip.lk_track_affine(ctx, fr[0], fr[1:], 1, opt=opt)
    plain = hip.lk_track(ctx, fr[0], fr[1:], opt)
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    _close(fr)
    for t in range(n_targets):
        what = (win, n_targets, arith, scene.MIX8[t])
        for k in range(3):      # the forward part is the oracle's in this mode
            _assert_same(plain[k][t], forward[t][k], "forward " + NAMES[k], what)
        for k, j in ((0, 0), (1, 1), (2, 2), (5, 3), (6, 4)):
            _assert_same(got[k][t], refined[t][j], NAMES[k], what)
    assert not got[3].any() and not got[4].any(), "no backward pass was asked for"


# ---- 2. option off ----
def test_affine_0_gives_the_bits_of_the_normalized_call_and_launches_nothing_new(ctx):
    win = 10
    kps = scene.keypoints(win)
    fr = _frames(ctx, win, [scene.frame1()] + scene.targets(win, 5), kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    for normalize, thr, fb in ((0, 0.0, 0.0), (0, 0.75, 1.0), (1, 0.75, 1.0)):
        want = hip.lk_track_normalized(ctx, fr[0], fr[1:], normalize, thr, fb, -1, opt)
        off = hip.lk_track_affine(ctx, fr[0], fr[1:], 0, normalize, thr, fb, -1, opt)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(off[:5], want)), (normalize, thr, fb)
        assert not off[5].any() and not off[6].any()
    ctx.enable_timing(True)
    counts = []
    for call in (lambda: hip.lk_track_normalized(ctx, fr[0], fr[1:], 0, 0.75, 1.0, -1, opt),
                 lambda: hip.lk_track_affine(ctx, fr[0], fr[1:], 0, 0, 0.75, 1.0, -1, opt),
                 lambda: hip.lk_track_affine(ctx, fr[0], fr[1:], 1, 0, 0.75, 1.0, -1, opt)):
        ctx.reset_timing()
        call()
        counts.append({k: v[0] for k, v in ctx.timing().items()})
    ctx.enable_timing(False)
    _close(fr)
    assert counts[0] == counts[1], counts
    assert counts[2] == {**counts[0], "lk": 2}, counts          # the refinement is timed under the forward launch's class
    assert counts[0]["lk"] == 1 and counts[0]["lk_fb"] == 1 and counts[0]["lk_corr"] == 1, counts


# ---- 3. the checks judge the refined end points ----
FB, THR = 1.0, 0.75


@pytest.mark.parametrize("win", [10, 21])
def test_forward_backward_and_minimum_correlation_judge_the_refined_rows(ctx, win):
    n_targets = 6
    kps, forward, refined = scene.reference(win, scene.MIX8, oracle.EMU_CANONICAL)
    oopt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    thr2 = fb_scene.thr2_of(FB)
    want, dropped_corr, dropped_fb, differs = [], 0, 0, 0
    with oracle.emulation(oracle.EMU_CANONICAL):
        p1 = oracle.Pyramid(np.array(scene.frame1()), win, MAX_LEVEL)
        for t in range(n_targets):
            gt = scene.target(scene.MIX8[t], win)
            q, st, err = refined[t][:3]
            keep, _ = corr_ref.rows(np.array(scene.frame1()), np.array(gt), win, kps, q, st, THR)
            idx = np.nonzero(keep == 1)[0]
            bxy, bst = np.zeros((len(kps), 2), np.float32), np.zeros(len(kps), np.uint8)
            b, sb, _ = oracle.lk(oracle.Pyramid(np.array(gt), win, MAX_LEVEL), p1, q[idx], oopt)
            bxy[idx], bst[idx] = b, sb
            dx, dy = bxy[:, 0] - kps[:, 0], bxy[:, 1] - kps[:, 1]
            with np.errstate(invalid="ignore", over="ignore"):
                final = ((keep == 1) & (bst == 1) & (dx * dx + dy * dy <= thr2)).astype(np.uint8)
            want.append((q, final, err, bxy, bst))
            dropped_corr += int((st == 1).sum() - keep.sum())
            dropped_fb += int(keep.sum() - final.sum())
            # what the same checks make of the UNREFINED rows, for the assertion that the composition matters
            c = fb_scene.composed(p1, oracle.Pyramid(np.array(gt), win, MAX_LEVEL), kps, oopt, FB)
            differs += int((c["status"] != final).sum())
    print(win, "dropped by the correlation", dropped_corr, "by the backward pass", dropped_fb, "final status differs from the unrefined rows'", differs)
    assert dropped_corr >= 5 and dropped_fb >= 5 and sum(int(w[1].sum()) for w in want) >= 50, "asserted on the reference"
    fr = _frames(ctx, win, [scene.frame1()] + scene.targets(win, n_targets), kps)
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    got = hip.lk_track_affine(ctx, fr[0], fr[1:], 1, 0, THR, FB, -1, hip.flow_options(window_size=win, max_level=MAX_LEVEL))
    _close(fr)
    for t in range(n_targets):
        for k in range(5):
            _assert_same(got[k][t], want[t][k], NAMES[k], (win, scene.MIX8[t]))
        _assert_same(got[6][t], refined[t][4], NAMES[6], (win, scene.MIX8[t]))


# ---- 4. arguments ----
def test_values_other_than_0_and_1_and_the_combination_with_normalize_are_refused(ctx):
    win = 10
    fr = _frames(ctx, win, [scene.frame1(), scene.target("rot", win)], scene.detected())
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    for value in (2, -1):
        with pytest.raises(hip.PolychaseHipError, match="affine"):
            hip.lk_track_affine(ctx, fr[0], fr[1:], value, opt=opt)
    with pytest.raises(hip.PolychaseHipError, match="normalize"):
        hip.lk_track_affine(ctx, fr[0], fr[1:], 1, 1, opt=opt)
    an = hip.Analyzer(ctx, scene.W, scene.H, hip.gftt_options(), opt)
    for value in (-1, 2):
        with pytest.raises(hip.PolychaseHipError, match="affine"):
            an.set_affine_refinement(value)
    an.set_normalize(1)
    with pytest.raises(hip.PolychaseHipError, match="normalize"):
        an.set_affine_refinement(1)
    an.set_normalize(0)
    an.set_affine_refinement(1)
    an.set_normalize(1)          # switched on behind the refinement: the job is refused
    an.put_frame(1, scene.rolling_clip(2)[0])
    an.put_frame(2, scene.rolling_clip(2)[1])
    with pytest.raises(hip.PolychaseHipError, match="normalize"):
        an.submit(1, [2])
    an.close()
    _close(fr)


# ---- 5. the analyzer ----
def test_analyzer_jobs_under_the_option_hold_the_reference_rows_and_show_two_lk_launches(ctx):
    win = 10
    frames = scene.rolling_clip(5)
    fopt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    oopt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    an = hip.Analyzer(ctx, scene.W, scene.H, hip.gftt_options(), fopt, ring_frames=17, max_jobs=3)
    for i, f in enumerate(frames):
        an.put_frame(i + 1, f)
    jobs = ((1, [2, 5], 1), (2, [3, 4, 5], 0), (1, [4], 1))      # a change between two submits affects only the later jobs
    launches = []
    out = []
    for f1, tg, v in jobs:
        an.set_affine_refinement(v)
        ctx.synchronize()
        ctx.enable_timing(["lk"])
        ctx.reset_timing()
        an.submit(f1, tg)
        out.append(an.collect())
        launches.append(ctx.timing()["lk"][0])
        ctx.enable_timing(False)
    an.close()
    assert launches == [2, 1, 2], launches
    moved = 0
    with oracle.emulation(oracle.EMU_CANONICAL):
        pyr = {i + 1: oracle.Pyramid(np.ascontiguousarray(f[:, :, 0]), win, MAX_LEVEL) for i, f in enumerate(frames)}
        for (f1, tg, v), (got_f1, kps, _, flows) in zip(jobs, out):
            assert got_f1 == f1 and len(kps) >= 10
            forward = [oracle.lk(pyr[f1], pyr[t], kps, oopt) for t in tg]
            want = ref.refine(ref.Planes(pyr[f1]), [ref.Planes(pyr[t]) for t in tg], kps, forward, oopt) if v else forward
            for t, w, f in zip(tg, want, forward):
                idx, xy, err = flows[t]
                sel = np.nonzero(w[1] == 1)[0]
                assert len(sel) >= 5 and np.array_equal(idx, sel.astype(np.uint32)), (f1, t, v)
                assert np.array_equal(_bits(xy), _bits(w[0][sel])) and np.array_equal(_bits(err), _bits(w[2][sel])), (f1, t, v)
                moved += int(v and w[0].tobytes() != f[0].tobytes())
    assert moved == 3, "every pair's rows under the option are refined ones"
