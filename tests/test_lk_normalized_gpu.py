"""GPU: brightness-normalised LK at stage and analyzer level (kernels_lk_norm.hip through pc_lk_track_normalized and
pc_analyzer_set_normalize) against the numpy restatement of the rule (tests/lk_normalized_ref.py), bit for bit, in both arithmetic
modes -- which must give the same bits: the rule has one instance.  The scenes are tests/lk_correlation_scene.py's 96 x 80 gray
frames; a test compares about 600 (keypoint, target) pairs with the reference."""
import functools

import numpy as np
import pytest

import lk_correlation_scene as scene
import lk_normalized_ref as ref
import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu

MODES = (hip.ARITH_CANONICAL, hip.ARITH_OPENCV_X86)
MAX_LEVEL = 2
BIAS = 17


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


def _in_both_modes(ctx, call):
    """call() under either arithmetic mode -> the canonical result, after asserting that the other mode gives the same bits"""
    out = []
    for m in MODES:
        ctx.set_arithmetic(m)
        out.append(call())
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes(), "the arithmetic mode plays no part in the normalised rule"
    return out[0]


@functools.lru_cache(maxsize=None)
def _planes(kind, win, seed=scene.TARGET_SEED):
    """reference planes of a scene frame: 'frame1', 'flat', or a kind of lk_correlation_scene.target"""
    return ref.Planes(oracle.Pyramid(np.array(_gray(kind, win, seed)), win, MAX_LEVEL))


@functools.lru_cache(maxsize=None)
def _gray(kind, win, seed=scene.TARGET_SEED):
    if kind == "frame1":
        return scene.frame1()
    if kind == "flat":
        return np.full((scene.H, scene.W), 128, np.uint8)        # vJ = 0 in every window: g = 1
    return scene.target(kind, win, seed)


def _mixed_keypoints(win, n):
    """n of lk_correlation_scene.keypoints: the sub-pixel, border and out-of-frame ones (42) and detected ones in front of them"""
    k = scene.keypoints(win)
    assert 42 <= n <= len(k)
    return k[len(k) - n:] if n > 42 else k[len(k) - 42:][:n]


def _assert_rows(got, want, what):
    for name, g, w in zip(("next_xy", "status", "err", "back_xy", "back_status"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        d = _bits(g) != _bits(w)
        bad = np.nonzero(d.reshape(len(w), d.size // max(1, len(w))).any(axis=1))[0]
        assert not len(bad), (what, name, "rows", bad[:8].tolist(), g[bad[:2]].tolist(), w[bad[:2]].tolist())


# ---- 1. bit parity ----
# eight targets with a flat one among them; 73 = 4 * 18 + 1 keypoints: the last workgroup holds one wavefront
KINDS8 = ("same", "shift", "gain", "unrelated", "border", "flat", "gain", "border")


SEEDS8 = tuple(scene.TARGET_SEED if i < 6 else scene.TARGET_SEED + 7 * i for i in range(8))


def _eight_targets_reference(win):
    kps = _mixed_keypoints(win, 73)
    oopt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    want = [ref.track(_planes("frame1", win), _planes(k, win, s), kps, oopt) for k, s in zip(KINDS8, SEEDS8)]
    st = np.stack([w[1] for w in want])
    print(win, "status 1 per target:", list(zip(KINDS8, st.sum(axis=1).tolist())))
    # asserted on the REFERENCE, before anything is compared with it: tracked and lost rows, off the integer grid, outside the frame
    assert st[0].sum() >= (40 if win > 3 else 10) and (st.sum(axis=1) < len(kps)).all() and not st[:, -4:].any()
    assert st[:, 31:55].any() and st[:, 55:64].any(), "sub-pixel and border keypoints track"
    return kps, want


@pytest.mark.parametrize("win", [3, 8, 10, 21, 31])
def test_eight_targets_match_the_reference(ctx, win):
    kps, want = _eight_targets_reference(win)
    fr = _frames(ctx, win, [_gray("frame1", win)] + [_gray(k, win, s) for k, s in zip(KINDS8, SEEDS8)], kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    got = _in_both_modes(ctx, lambda: hip.lk_track_normalized(ctx, fr[0], fr[1:], 1, opt=opt)[:3])
    for t in range(8):
        _assert_rows([a[t] for a in got], want[t], (win, KINDS8[t]))
    _close(fr)


@pytest.mark.parametrize("n_kps", [0, 1, 65])
@pytest.mark.parametrize("n_targets", [1, 3])
@pytest.mark.parametrize("win,max_level", [(10, 0), (31, 2)])
def test_target_and_keypoint_counts_and_level_zero_alone(ctx, win, max_level, n_targets, n_kps):
    kps = _mixed_keypoints(win, 65)[:n_kps]
    kinds = ("shift", "gain", "border")[:n_targets]
    fr = _frames(ctx, win, [_gray("frame1", win)] + [_gray(k, win) for k in kinds], kps)
    opt = hip.flow_options(window_size=win, max_level=max_level)
    oopt = oracle.flow_options(window_size=win, max_level=max_level)
    got = _in_both_modes(ctx, lambda: hip.lk_track_normalized(ctx, fr[0], fr[1:], 1, opt=opt)[:3])
    assert got[0].shape == (n_targets, n_kps, 2) and got[1].shape == (n_targets, n_kps)
    for t, k in enumerate(kinds):
        want = ref.track(_planes("frame1", win), _planes(k, win), kps, oopt)
        assert n_kps < 65 or 0 < want[1].sum() < n_kps
        _assert_rows([a[t] for a in got], want, (win, max_level, k, n_kps))
    _close(fr)


# ---- 2. forward-backward: both passes under the rule ----
FB_THRESHOLD = 1.0
FB_KINDS = ("shift", "gain", "border")


def _forward_backward_reference(win):
    kps = _mixed_keypoints(win, 101)
    oopt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    want = []
    for k in FB_KINDS:
        fwd = ref.track(_planes("frame1", win), _planes(k, win), kps, oopt)
        w = ref.forward_backward(_planes("frame1", win), _planes(k, win), kps, oopt, FB_THRESHOLD, forward=fwd)
        alive, kept = int(fwd[1].sum()), int(w[1].sum())
        print(win, k, "forward", alive, "kept", kept, "backward status 1", int(w[4].sum()))
        assert 0 < kept < alive, "the check must drop some rows and keep some (asserted on the reference)"
        want.append(w)
    return kps, want


@pytest.mark.parametrize("win", [10, 21])
def test_forward_backward_check_runs_the_normalised_backward_pass(ctx, win):
    kps, want = _forward_backward_reference(win)
    fr = _frames(ctx, win, [_gray("frame1", win)] + [_gray(k, win) for k in FB_KINDS], kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    got = _in_both_modes(ctx, lambda: hip.lk_track_normalized(ctx, fr[0], fr[1:], 1, 0.0, FB_THRESHOLD, opt=opt))
    for t, k in enumerate(FB_KINDS):
        _assert_rows([a[t] for a in got], want[t], (win, k))
    _close(fr)


# ---- 3. a bias changes nothing, exactly -- with the option, and only with it ----
@pytest.mark.parametrize("win", [8, 10])
def test_a_bias_on_the_target_changes_no_bit_of_the_normalised_rows(ctx, win):
    f1 = scene.gain(scene.frame1(), 0.8, 20.0)
    ft = scene.gain(scene.target("shift", win), 0.8, 20.0)
    assert int(ft.max()) + BIAS <= 255, "nothing may clip"
    kps = scene.keypoints(win)
    fr = _frames(ctx, win, [f1, ft, ft + np.uint8(BIAS)], kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    on = hip.lk_track_normalized(ctx, fr[0], fr[1:], 1, opt=opt)
    off = hip.lk_track_normalized(ctx, fr[0], fr[1:], 0, opt=opt)
    assert on[1][0].sum() >= 10
    assert on[0][0].tobytes() == on[0][1].tobytes() and on[1][0].tobytes() == on[1][1].tobytes()
    assert off[0][0].tobytes() != off[0][1].tobytes(), "plain LK is displaced by the bias"
    _close(fr)


# ---- 4. option off ----
def test_option_off_is_the_correlated_call_and_launches_nothing_new(ctx):
    win = 10
    kps, tgts = scene.keypoints(win), scene.targets(win, 5)
    fr = _frames(ctx, win, [scene.frame1()] + tgts, kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    for thr, fb in ((0.0, 0.0), (0.75, 1.0)):
        corr = hip.lk_track_correlated(ctx, fr[0], fr[1:], thr, fb, -1, opt, corr=False)
        off = hip.lk_track_normalized(ctx, fr[0], fr[1:], 0, thr, fb, -1, opt)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(off[:3], corr[:3])), (thr, fb)
    back = hip.lk_track_fb(ctx, fr[0], fr[1:], 1.0, opt)
    off = hip.lk_track_normalized(ctx, fr[0], fr[1:], 0, 0.0, 1.0, -1, opt)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off, back)), "... plus the back outputs of pc_lk_track_fb"
    on = hip.lk_track_normalized(ctx, fr[0], fr[1:], 1, 0.0, 1.0, -1, opt)
    assert on[0].tobytes() != off[0].tobytes()
    ctx.enable_timing(True)
    counts = []
    for call in (lambda: hip.lk_track_correlated(ctx, fr[0], fr[1:], 0.75, 1.0, -1, opt, corr=False),
                 lambda: hip.lk_track_normalized(ctx, fr[0], fr[1:], 0, 0.75, 1.0, -1, opt),
                 lambda: hip.lk_track_normalized(ctx, fr[0], fr[1:], 1, 0.75, 1.0, -1, opt)):
        ctx.reset_timing()
        call()
        counts.append({k: v[0] for k, v in ctx.timing().items()})
    ctx.enable_timing(False)
    assert counts[0] == counts[1] == counts[2], counts        # the normalised launches take the places of the plain ones
    assert counts[0]["lk"] == 1 and counts[0]["lk_fb"] == 1 and counts[0]["lk_corr"] == 1, counts
    _close(fr)


# ---- 5. arguments ----
def test_values_other_than_0_and_1_are_refused(ctx):
    win = 10
    fr = _frames(ctx, win, [scene.frame1(), scene.target("shift", win)], scene.detected())
    for value in (2, -1):
        with pytest.raises(hip.PolychaseHipError, match="normalize"):
            hip.lk_track_normalized(ctx, fr[0], fr[1:], value, opt=hip.flow_options(window_size=win, max_level=MAX_LEVEL))
    an = hip.Analyzer(ctx, scene.W, scene.H, hip.gftt_options(), hip.flow_options(window_size=win, max_level=MAX_LEVEL))
    for value in (-1, 2):
        with pytest.raises(hip.PolychaseHipError, match="normalize"):
            an.set_normalize(value)
    an.close()
    _close(fr)


# ---- the analyzer: its rows are the stage-level call's ----
def test_analyzer_jobs_submitted_under_the_option_hold_the_stage_level_rows(ctx):
    import fb_scene

    win, fb = 10, 1.0
    frames = fb_scene.clip(scene.W, scene.H, 4)
    frames = [f if i % 2 == 0 else np.ascontiguousarray(np.repeat(scene.gain(f[:, :, 0], 0.7, 30.0)[:, :, None], 3, axis=2))
              for i, f in enumerate(frames)]
    fopt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    an = hip.Analyzer(ctx, scene.W, scene.H, hip.gftt_options(), fopt, ring_frames=17, max_jobs=3)
    an.set_fb_threshold(fb)
    for i, f in enumerate(frames):
        an.put_frame(i + 1, f)
    jobs = ((1, [2, 3], 1), (2, [3, 4], 0), (1, [4], 1))      # a change between two submits affects only the later jobs
    for f1, tg, v in jobs:
        an.set_normalize(v)
        an.submit(f1, tg)
    out = [an.collect() for _ in jobs]
    an.close()
    differs = 0
    for (f1, tg, v), (got_f1, kps, _, flows) in zip(jobs, out):
        assert got_f1 == f1 and len(kps) >= 10
        fr = _frames(ctx, win, [frames[f1 - 1][:, :, 0]] + [frames[t - 1][:, :, 0] for t in tg], kps)
        stage = {n: hip.lk_track_normalized(ctx, fr[0], fr[1:], n, 0.0, fb, -1, fopt) for n in (0, 1)}
        for k, t in enumerate(tg):
            idx, xy, err = flows[t]
            sel = np.nonzero(stage[v][1][k] == 1)[0]
            assert len(sel) >= 5 and np.array_equal(idx, sel.astype(np.uint32)), (f1, t, v)
            assert np.array_equal(_bits(xy), _bits(stage[v][0][k][sel])) and np.array_equal(_bits(err), _bits(stage[v][2][k][sel])), (f1, t, v)
            differs += stage[0][0][k].tobytes() != stage[1][0][k].tobytes()
        _close(fr)
    assert differs == 5, "every pair's rows depend on the option"
