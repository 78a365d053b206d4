"""GPU: minimum correlation at stage and analyzer level (kernels_lk_corr.hip through pc_lk_track_correlated and
pc_analyzer_set_min_correlation) against the numpy restatement of the rule (tests/lk_correlation_ref.py), bit for bit in both
arithmetic modes; the scenes are tests/lk_correlation_scene.py's 96 x 80 gray frames."""
import numpy as np
import pytest

import fb_scene
import lk_correlation_ref as ref
import lk_correlation_scene as scene
import oracle
import target_mask_ref
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ARITH = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL), "opencv_x86": (hip.ARITH_OPENCV_X86, oracle.EMU_OPENCV_X86)}
MAX_LEVEL = 2
THRESHOLDS = (0.75, 0.95)
SCORE_TOL = 2.0 ** -23      # the decision uses no division or root; the score can differ by a double-rounding flip of the last fp32 bit


@pytest.fixture(scope="module", params=sorted(ARITH))
def actx(request):
    c = hip.Context(0)
    c.set_arithmetic(ARITH[request.param][0])
    yield request.param, c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _frames(ctx, win, grays, kps):
    fr = []
    for g in grays:
        f = hip.Frame(ctx, scene.W, scene.H, win, MAX_LEVEL)
        f.set_gray(np.array(g))
        fr.append(f)
    fr[0].set_keypoints(np.array(kps))
    return fr


def _close(fr):
    for f in fr:
        f.close()


def _reference(win, tgts, kps, xy0, st0, thr):
    """per target: (keep, score) of the rule on the forward call's own rows"""
    return [ref.rows(scene.frame1(), tgts[t], win, kps, xy0[t], st0[t], thr) for t in range(len(tgts))]


def _assert_parity(got, xy0, st0, err0, want, what):
    xy, st, err, sc = got
    assert np.array_equal(_bits(xy), _bits(xy0)) and np.array_equal(_bits(err), _bits(err0)), (what, "next_xy and err stay")
    for t, (k, s) in enumerate(want):
        assert np.array_equal(st[t], st0[t] & k), (what, t, "status", int((st[t] != (st0[t] & k)).sum()))
        if sc is not None:
            d = np.abs(sc[t].astype(np.float64) - s.astype(np.float64))
            assert d.max(initial=0.0) <= SCORE_TOL, (what, t, "score", float(d.max()))
            assert not sc[t][st0[t] == 0].any(), (what, t, "the score is 0 where the record reached the pass with status 0")


# ---- stage parity ----
@pytest.mark.parametrize("win", scene.WINDOWS)
def test_eight_targets_match_the_reference(actx, win):
    arith, ctx = actx
    kps, tgts = scene.keypoints(win), scene.targets(win, 8)
    n_det = len(scene.detected())
    fr = _frames(ctx, win, [scene.frame1()] + tgts, kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    xy0, st0, err0 = hip.lk_track(ctx, fr[0], fr[1:], opt)
    want = {thr: _reference(win, tgts, kps, xy0, st0, thr) for thr in THRESHOLDS}
    # the scene must exercise both outcomes: asserted on the REFERENCE's result, before anything is compared with it
    for t, kind in enumerate(scene.MIX8):
        k = want[0.75][t][0]
        print(win, arith, t, kind, "forward", int(st0[t].sum()), "kept at 0.75", int(k.sum()), "at 0.95", int(want[0.95][t][0].sum()))
        if kind == "shift":
            scene.check_fractions(int(st0[t].sum()), int(k.sum()), (win, arith, t))
        if kind == "same":
            assert np.array_equal(k, st0[t]) and st0[t].sum() >= n_det
        if kind == "unrelated" and win >= 10:
            assert st0[t].sum() >= 10 and not k.any()
    if win != 3:            # (window 3 with the gain scene: only 3 forward rows)
        scene.check_fractions(int(st0[2].sum()), int(want[0.75][2][0].sum()), (win, arith, "gain"))
    extra = st0[0][n_det:]                                       # the 'same' target: sub-pixel, border and outside keypoints
    assert extra[:24].all() and extra[24:33].any(), "sub-pixel and near-border keypoints track"
    assert win == 3 or extra[33:38].any(), "... and so do keypoints just outside the frame, whose windows lie partly in the padding"
    assert not st0[:, -4:].any(), "keypoints whose template window fails the bounds test never do"
    assert (xy0[st0 == 1] != np.floor(xy0[st0 == 1])).any()
    for thr in THRESHOLDS:
        _assert_parity(hip.lk_track_correlated(ctx, fr[0], fr[1:], thr, opt=opt), xy0, st0, err0, want[thr], (win, arith, thr))
    _close(fr)


@pytest.mark.parametrize("n_kps", [1, 63, 65])
@pytest.mark.parametrize("n_targets", [1, 3])
@pytest.mark.parametrize("win", [10, 31])
def test_target_and_keypoint_counts(actx, win, n_targets, n_kps):
    arith, ctx = actx
    kps = scene.keypoints(win)[len(scene.detected()) - 40:][:n_kps]        # detected, sub-pixel and border ones
    tgts = scene.targets(win, 3)[:n_targets]                               # same; same, shift, gain
    fr = _frames(ctx, win, [scene.frame1()] + tgts, kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    xy0, st0, err0 = hip.lk_track(ctx, fr[0], fr[1:], opt)
    assert st0.shape == (n_targets, n_kps) and st0.any()
    want = _reference(win, tgts, kps, xy0, st0, 0.75)
    _assert_parity(hip.lk_track_correlated(ctx, fr[0], fr[1:], 0.75, opt=opt), xy0, st0, err0, want, (win, n_targets, n_kps))
    _close(fr)


# ---- equivalences ----
def test_threshold_zero_is_the_masked_call_and_with_scores_drops_nothing(actx):
    arith, ctx = actx
    win = 10
    kps, tgts = scene.keypoints(win), scene.targets(win, 5)
    fr = _frames(ctx, win, [scene.frame1()] + tgts, kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    masked = hip.lk_track_masked(ctx, fr[0], fr[1:], 0.0, -1, opt)
    off = hip.lk_track_correlated(ctx, fr[0], fr[1:], 0.0, opt=opt, corr=False)
    assert off[3] is None and all(a.tobytes() == b.tobytes() for a, b in zip(off[:3], masked))
    xy, st, err, sc = hip.lk_track_correlated(ctx, fr[0], fr[1:], 0.0, opt=opt)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((xy, st, err), masked)), "the pass only writes scores"
    on = hip.lk_track_correlated(ctx, fr[0], fr[1:], 0.75, opt=opt)
    assert on[3].tobytes() == sc.tobytes() and int(on[1].sum()) < int(st.sum())
    want = _reference(win, tgts, kps, masked[0], masked[1], 0.0)
    _assert_parity((xy, st, err, sc), masked[0], masked[1], masked[2], want, "threshold 0")
    # the launch belongs to a timed class of its own, and is absent when nothing asks for it
    ctx.enable_timing(True)
    counts = []
    for thr, corr in ((0.0, False), (0.0, True), (0.75, False)):
        ctx.reset_timing()
        hip.lk_track_correlated(ctx, fr[0], fr[1:], thr, opt=opt, corr=corr)
        counts.append({k: v[0] for k, v in ctx.timing().items()})
    ctx.enable_timing(False)
    assert "lk_corr" not in counts[0], "Context.timing() lists the class once it has launched"
    assert [c.get("lk_corr", 0) for c in counts] == [0, 1, 1] and all(c["lk"] == 1 and c["lk_fb"] == 0 for c in counts), counts
    _close(fr)


# ---- combination ----
def test_with_a_target_mask_and_the_forward_backward_check_the_status_is_the_and_of_the_three(actx):
    arith, ctx = actx
    win, margin, fb = 10, 3, 1.0
    kinds = ("shift", "gain", "border")
    kps = np.array(scene.detected())
    tgts = [scene.target(k, win) for k in kinds]
    masks = []
    for k in kinds:                 # off over the target's occluder rectangle (fb_scene.occluded)
        m = np.full((scene.H, scene.W), 200, np.uint8)
        x0, y0 = (0.1, 0.5) if k == "border" else (0.3, 0.3)
        rx, ry = int(scene.W * x0), int(scene.H * y0)
        m[ry:ry + scene.H // 3, rx:rx + scene.W // 3] = 0
        masks.append(m)
    fr = _frames(ctx, win, [scene.frame1()] + tgts, kps)
    for f, m in zip(fr[1:], masks):
        f.set_mask(m)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    xy0, st0, err0 = hip.lk_track(ctx, fr[0], fr[1:], opt)
    oopt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    want = []
    with oracle.emulation(ARITH[arith][1]):
        p1 = oracle.Pyramid(np.array(scene.frame1()), win, MAX_LEVEL)
        for t, g in enumerate(tgts):
            c = fb_scene.composed(p1, oracle.Pyramid(np.array(g), win, MAX_LEVEL), kps, oopt, fb)
            assert np.array_equal(c["status_f"], st0[t]) and np.array_equal(_bits(c["next_xy"]), _bits(xy0[t]))
            by_mask = target_mask_ref.keep(xy0[t], st0[t], masks[t], margin)
            by_corr, _ = ref.rows(scene.frame1(), g, win, kps, xy0[t], st0[t], 0.75)
            by_fb = c["status"]
            alive = int(st0[t].sum())
            print(arith, kinds[t], "forward", alive, "mask", int(by_mask.sum()), "correlation", int(by_corr.sum()), "fb", int(by_fb.sum()))
            for part in (by_mask, by_corr, by_fb):
                assert 0 < int(part.sum()) < alive, "every check drops some rows and keeps some"
            want.append(by_mask & by_corr & by_fb)
    xy, st, err, sc = hip.lk_track_correlated(ctx, fr[0], fr[1:], 0.75, fb, margin, opt)
    assert np.array_equal(_bits(xy), _bits(xy0)) and np.array_equal(_bits(err), _bits(err0))
    for t in range(len(kinds)):
        assert np.array_equal(st[t], want[t]), (kinds[t], int((st[t] != want[t]).sum()))
    _close(fr)


# ---- errors ----
@pytest.mark.parametrize("value", [float("nan"), -0.1, 1.5])
def test_bad_values_raise(actx, value):
    arith, ctx = actx
    win = 10
    fr = _frames(ctx, win, [scene.frame1(), scene.target("shift", win)], scene.detected())
    with pytest.raises(hip.PolychaseHipError, match="min_correlation"):
        hip.lk_track_correlated(ctx, fr[0], fr[1:], value, opt=hip.flow_options(window_size=win, max_level=MAX_LEVEL))
    an = hip.Analyzer(ctx, scene.W, scene.H, hip.gftt_options(), hip.flow_options(window_size=win, max_level=MAX_LEVEL))
    with pytest.raises(hip.PolychaseHipError, match="min_correlation"):
        an.set_min_correlation(value)
    an.close()
    _close(fr)


# ---- the analyzer ----
def _gain_clip(n):
    """fb_scene.clip (R = G = B, so gray is the channel) with every second frame x 0.7 + 30"""
    frames = fb_scene.clip(scene.W, scene.H, n)
    return [f if i % 2 == 0 else np.ascontiguousarray(np.repeat(scene.gain(f[:, :, 0], 0.7, 30.0)[:, :, None], 3, axis=2))
            for i, f in enumerate(frames)]


def test_analyzer_rows_are_the_threshold_zero_rows_filtered_by_the_reference():
    win = 10
    ctx = hip.Context(0)
    frames = _gain_clip(4)
    gray = [np.ascontiguousarray(f[:, :, 0]) for f in frames]
    fopt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)

    def run(values):
        """jobs 1 -> (2, 3) and 2 -> (3, 4), each submitted under its value"""
        an = hip.Analyzer(ctx, scene.W, scene.H, hip.gftt_options(), fopt, ring_frames=17, max_jobs=3)
        for i, f in enumerate(frames):
            an.put_frame(i + 1, f)
        for (f1, tg), v in zip(((1, [2, 3]), (2, [3, 4])), values):
            if v is not None:
                an.set_min_correlation(v)
            an.submit(f1, tg)
        out = [an.collect() for _ in range(2)]
        an.close()
        return out

    plain = run((None, None))
    got = run((0.75, 0.0))           # a change between two submits affects only the later job
    late = run((None, 0.75))
    for job in range(2):
        f1, kps, detected, flows = plain[job]
        assert got[job][0] == late[job][0] == f1 and np.array_equal(got[job][1], kps) and np.array_equal(late[job][1], kps)
        for t, (idx, xy, err) in flows.items():
            q, st = np.zeros((len(kps), 2), np.float32), np.zeros(len(kps), np.uint8)
            q[idx], st[idx] = xy, 1
            k, _ = ref.rows(gray[f1 - 1], gray[t - 1], win, kps, q, st, 0.75)
            sel = k[idx] == 1
            print("job", f1, "->", t, "rows", len(idx), "kept", int(sel.sum()))
            scene.check_fractions(len(idx), int(sel.sum()), (f1, t))
            for res, filtered in ((got, job == 0), (late, job == 1)):
                gi, gxy, gerr = res[job][3][t]
                wi, wxy, werr = (idx[sel], xy[sel], err[sel]) if filtered else (idx, xy, err)
                assert np.array_equal(gi, wi) and np.array_equal(_bits(gxy), _bits(wxy)) and np.array_equal(_bits(gerr), _bits(werr)), (f1, t, filtered)
    ctx.close()
