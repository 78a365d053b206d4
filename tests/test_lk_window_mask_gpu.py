"""GPU: masked LK windows at stage and analyzer level (kernels_mask.hip's weight planes, kernels_lk_wmask.hip through
pc_lk_track_window_masked and pc_analyzer_set_mask_windows) against the numpy restatement of the rule
(tests/lk_window_mask_ref.py), bit for bit, in both arithmetic modes.  The frames are tests/lk_window_mask_scene.py's two-layer
scene cut to 161 x 119: odd sizes, and the disc's outline leaves through the bottom border."""
import functools

import numpy as np
import pytest

import lk_window_mask_ref as ref
import lk_window_mask_scene as scene
import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu

W, H = 161, 119
MAX_LEVEL = 2
MODES = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL, False), "x86": (hip.ARITH_OPENCV_X86, oracle.EMU_LK_SIMD, True)}
TIMES8 = (1, 2, 3, 4, 0.5, 1.5, 2.5, -1)
FB_THRESHOLD = 1.0


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_arithmetic(hip.ARITH_CANONICAL)
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@functools.lru_cache(maxsize=None)
def _frame(k):
    g, m = scene.frame(k)
    return np.ascontiguousarray(g[:H, :W]), np.ascontiguousarray(m[:H, :W])


@functools.lru_cache(maxsize=None)
def _planes(k, win, max_level=MAX_LEVEL):
    p = oracle.Pyramid(_frame(k)[0], win, max_level)
    assert [p.level_size(l) for l in range(p.num_levels)] == ref.level_sizes(W, H, win, max_level)
    return ref.Planes(p)


@functools.lru_cache(maxsize=None)
def _weights(k, win, max_level=MAX_LEVEL):
    return ref.weight_pyramid(_frame(k)[1], win, ref.level_sizes(W, H, win, max_level))


def _keypoints(win, n=65):
    """in the band first (touched), then deep inside, on the outline, outside the mask, at the frame border, out of the frame;
    all but a few off the integer grid"""
    c = scene.CENTRE
    band = scene.ring_keypoints(0.0, win / 2, 38)
    deep = np.array([(c[0] + dx, c[1] + dy) for dx, dy in ((0, 0), (3.25, -2.5), (-4, 2.75), (2.5, 4), (-3, -4))])
    outline = scene.ring_keypoints(0.0, 0.0, 4)
    outside = scene.ring_keypoints(-20.0, -2.0, 8)
    border = np.array([(0.4, 60.2), (160.0, 3.0), (96.3, 118.0), (150.7, 117.6), (0.0, 0.0), (80.5, 0.25)])
    gone = np.array([(-3.5, 50.0), (W + 4.2, 20.0), (30.5, -6.75), (-40.0, -40.0)])
    k = np.concatenate([band, deep, outline, outside, border, gone]).astype(np.float32)
    assert len(k) == 65
    return k[:n]


def _frames(ctx, win, times, kps, masks="own", max_level=MAX_LEVEL):
    """masks: 'own' = every frame under its disc, or one entry per frame: None (no mask), a plane, or 'own'"""
    fr = []
    for i, k in enumerate(times):
        f = hip.Frame(ctx, W, H, win, max_level)
        f.set_gray(_frame(k)[0])
        m = masks if isinstance(masks, str) else masks[i]
        if m is not None:
            f.set_mask(_frame(k)[1] if isinstance(m, str) else m)
        fr.append(f)
    fr[0].set_keypoints(np.array(kps, np.float32).reshape(-1, 2))
    return fr


def _close(fr):
    for f in fr:
        f.close()


def _assert_rows(got, want, what, names=("next_xy", "status", "err", "back_xy", "back_status")):
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        d = _bits(g) != _bits(w)
        bad = np.nonzero(d.reshape(len(w), d.size // max(1, len(w))).any(axis=1))[0]
        assert not len(bad), (what, name, "rows", bad[:8].tolist(), g[bad[:2]].tolist(), w[bad[:2]].tolist())


# ---- 1. the weight planes ----
def _mask_of(kind):
    disc = _frame(0)[1]
    if kind == "disc":
        return disc
    if kind == "borders":
        m = np.full((H, W), 7, np.uint8)              # any non-zero byte is on
        m[0, 0] = m[H - 1, W - 1] = m[0, 77] = m[60, 0] = m[H - 1, 30] = m[41, W - 1] = m[1, W - 2] = 0
        m[50, 80] = 0
        return m
    if kind == "all_on":
        return np.full((H, W), 255, np.uint8)
    assert kind == "all_off"
    return np.zeros((H, W), np.uint8)


@pytest.mark.parametrize("kind,win", [("disc", 10), ("disc", 31), ("polygon", 21), ("borders", 3), ("borders", 10), ("all_on", 8), ("all_off", 8)])
def test_weight_planes_match_the_restatement(ctx, kind, win):
    f = hip.Frame(ctx, W, H, win, 3)
    f.set_gray(_frame(0)[0])
    if kind == "polygon":
        f.set_mask_polygons([np.array([(20.5, 10.25), (150.0, 30.0), (170.0, 100.5), (60.0, 130.0), (-5.0, 70.0)], np.float32),
                             np.array([(100.0, 0.0), (161.0, 0.0), (161.0, 12.0)], np.float32)])
        mask = f.mask()
        assert 0 < (mask != 0).sum() < mask.size
    else:
        mask = _mask_of(kind)
        f.set_mask(mask)
    sizes = ref.level_sizes(W, H, win, 3)
    assert f.num_levels == len(sizes) and len(sizes) >= 2
    want = ref.weight_pyramid(mask, win, sizes)
    for l in range(len(sizes)):
        got = f.window_weights(l)
        assert set(np.unique(got).tolist()) <= {0, 255}
        assert np.array_equal(got != 0, want[l]), (kind, win, l, np.argwhere((got != 0) != want[l])[:4].tolist())
    # a change of the mask reaches the planes
    f.set_mask(np.full((H, W), 255, np.uint8))
    assert f.window_weights(len(sizes) - 1).all()
    f.set_mask(None)
    with pytest.raises(hip.PolychaseHipError, match="no mask"):
        f.window_weights(0)
    f.close()


# ---- 2. stage-level rows ----
@functools.lru_cache(maxsize=None)
def _eight_targets_reference(win, mode):
    kps = _keypoints(win)
    oopt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    with oracle.emulation(MODES[mode][1]):
        plain = oracle.lk(oracle.Pyramid(_frame(0)[0], win, MAX_LEVEL), oracle.Pyramid(_frame(1)[0], win, MAX_LEVEL), kps, oopt)
    want = [ref.track(_planes(0, win), _planes(k, win), kps, oopt, weights=_weights(0, win), x86=MODES[mode][2]) for k in TIMES8]
    st, touched = np.stack([w[1] for w in want]), want[0][3]
    print(win, mode, "status 1 per target:", st.sum(axis=1).tolist(), "touched", int(touched.sum()))
    # asserted on the REFERENCE, before anything is compared with it
    assert all(np.array_equal(w[3], touched) for w in want), "touched depends on frame1 and the keypoint alone"
    assert touched[:38].sum() >= 30 and touched.sum() >= 40, "the band is touched (but where the disc leaves the frame)"
    assert win > 10 or not touched[38:43].any(), "deep inside is not, below the window where the top level reaches the outline"
    assert (st.sum(axis=1) >= 8).all() and not st[:, -1].any(), "tracked rows, and a keypoint far outside fails"
    changed = (_bits(want[0][0]) != _bits(plain[0])).any(axis=1)
    assert changed[touched == 1].sum() >= 20 and not changed[touched == 0].any(), "the rule moves touched rows and no other"
    return kps, want


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("win", [3, 8, 10, 21, 31])
def test_eight_targets_match_the_restatement(ctx, win, mode):
    kps, want = _eight_targets_reference(win, mode)
    fr = _frames(ctx, win, (0,) + TIMES8, kps)
    ctx.set_arithmetic(MODES[mode][0])
    got = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, opt=hip.flow_options(window_size=win, max_level=MAX_LEVEL))
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    assert np.array_equal(got[5], want[0][3]), "touched"
    for t in range(8):
        _assert_rows([a[t] for a in got[:3]], want[t][:3], (win, mode, TIMES8[t]))
    _close(fr)


@pytest.mark.parametrize("n_kps", [0, 1, 65])
@pytest.mark.parametrize("n_targets", [1, 3])
@pytest.mark.parametrize("win,max_level", [(10, 0), (21, 2)])
def test_target_and_keypoint_counts_and_level_zero_alone(ctx, win, max_level, n_targets, n_kps):
    kps = _keypoints(win, n_kps)
    times = (1, 2.5, -1)[:n_targets]
    fr = _frames(ctx, win, (0,) + times, kps, max_level=max_level)
    opt = hip.flow_options(window_size=win, max_level=max_level)
    oopt = oracle.flow_options(window_size=win, max_level=max_level)
    for mode in sorted(MODES):
        ctx.set_arithmetic(MODES[mode][0])
        got = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, opt=opt)
        ctx.set_arithmetic(hip.ARITH_CANONICAL)
        assert got[0].shape == (n_targets, n_kps, 2) and got[1].shape == (n_targets, n_kps) and got[5].shape == (n_kps,)
        for t, k in enumerate(times):
            want = ref.track(_planes(0, win, max_level), _planes(k, win, max_level), kps, oopt, weights=_weights(0, win, max_level),
                             x86=MODES[mode][2])
            assert n_kps == 0 or want[3][0] == 1
            _assert_rows([a[t] for a in got[:3]], want[:3], (win, max_level, mode, k, n_kps))
            assert np.array_equal(got[5], want[3])
    _close(fr)


# ---- 3. the anchor: no off sample, today's bits ----
@pytest.mark.parametrize("win", [10, 21])
def test_all_on_mask_and_no_mask_on_frame1_give_the_plain_rows(ctx, win):
    kps = _keypoints(win)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    all_on = np.full((H, W), 255, np.uint8)
    for masks in ([all_on, all_on, None, all_on], [None, None, None, None], [None, "own", None, all_on]):
        fr = _frames(ctx, win, (0, 1, 2, -1), kps, masks)
        want = hip.lk_track_fb(ctx, fr[0], fr[1:], FB_THRESHOLD, opt)
        got = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, FB_THRESHOLD, -1, opt)
        if masks[1] is None or masks[1] is all_on:
            _assert_rows(got[:5], want, (win, "plain"))
        else:   # frame1 has no weights: the forward rows are the plain ones whatever the targets carry
            assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
        assert want[1].sum() >= 60 and not got[5].any()
        _close(fr)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_untouched_keypoints_of_a_mixed_job_keep_the_product_kernels_records(ctx, mode):
    win = 10
    kps = _keypoints(win)
    fr = _frames(ctx, win, (0, 1, 2, 3), kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    ctx.set_arithmetic(MODES[mode][0])
    plain = hip.lk_track(ctx, fr[0], fr[1:], opt)
    got = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, opt=opt)
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    touched = got[5] == 1
    assert 40 <= touched.sum() < 65
    for a, b in zip(got[:3], plain):
        assert a[:, ~touched].tobytes() == b[:, ~touched].tobytes()
    assert (_bits(got[0])[:, touched] != _bits(plain[0])[:, touched]).any(axis=2).sum() >= 60
    _close(fr)


# ---- 4. option off ----
def test_option_off_is_the_masked_call_and_launches_nothing_new(ctx):
    win = 10
    kps = _keypoints(win)
    fr = _frames(ctx, win, (0, 1, 2), kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    for fb, margin in ((0.0, -1), (FB_THRESHOLD, -1), (FB_THRESHOLD, 2)):
        masked = hip.lk_track_masked(ctx, fr[0], fr[1:], fb, margin, opt)
        off = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 0, fb, margin, opt)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(off[:3], masked)), (fb, margin)
        assert not off[5].any()
    back = hip.lk_track_fb(ctx, fr[0], fr[1:], FB_THRESHOLD, opt)
    off = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 0, FB_THRESHOLD, -1, opt)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off[:5], back)), "... plus the back outputs of pc_lk_track_fb"
    ctx.enable_timing(True)
    counts = []
    for call in (lambda: hip.lk_track_masked(ctx, fr[0], fr[1:], FB_THRESHOLD, 2, opt),
                 lambda: hip.lk_track_window_masked(ctx, fr[0], fr[1:], 0, FB_THRESHOLD, 2, opt),
                 lambda: hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, FB_THRESHOLD, 2, opt)):
        ctx.reset_timing()
        call()
        counts.append({k: v[0] for k, v in ctx.timing().items()})
    ctx.enable_timing(False)
    assert counts[0] == counts[1], counts
    assert counts[0]["lk"] == 1 and counts[0]["lk_fb"] == 1, counts
    # on: the masked launch behind the forward one; the weighted backward launch takes the plain one's place
    assert counts[2]["lk"] == 2 and counts[2]["lk_fb"] == 1, counts
    assert {k: v for k, v in counts[2].items() if k != "lk"} == {k: v for k, v in counts[0].items() if k != "lk"}, counts
    _close(fr)


# ---- 5. forward-backward: each pass under the weights of its template image ----
@functools.lru_cache(maxsize=None)
def _forward_backward_reference(win, mode):
    kps = _keypoints(win)
    oopt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    want = []
    for k, masked in ((1, True), (2, False), (-1, True)):
        w = ref.forward_backward(_planes(0, win), _planes(k, win), kps, oopt, FB_THRESHOLD, _weights(0, win),
                                 _weights(k, win) if masked else None, x86=MODES[mode][2])
        plain_back = ref.forward_backward(_planes(0, win), _planes(k, win), kps, oopt, FB_THRESHOLD, _weights(0, win), None,
                                          x86=MODES[mode][2])
        differ = int((_bits(w[3]) != _bits(plain_back[3])).any(axis=1).sum())
        print(win, mode, k, "kept", int(w[1].sum()), "backward status 1", int(w[4].sum()), "rows the target's weights move", differ)
        assert 10 <= w[1].sum() and w[4].sum() < len(kps)
        assert (differ >= 5) == masked, "the target's weights matter (asserted on the reference)"
        want.append(w)
    return kps, want


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("win", [10, 21])
def test_forward_backward_check_weights_the_backward_pass_of_masked_targets_only(ctx, win, mode):
    kps, want = _forward_backward_reference(win, mode)
    fr = _frames(ctx, win, (0, 1, 2, -1), kps, ["own", "own", None, "own"])
    ctx.set_arithmetic(MODES[mode][0])
    got = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, FB_THRESHOLD, -1, hip.flow_options(window_size=win, max_level=MAX_LEVEL))
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    for t in range(3):
        _assert_rows([a[t] for a in got[:5]], want[t], (win, mode, t))
    _close(fr)


def test_target_side_margin_composes_with_the_option(ctx):
    win = 10
    kps = _keypoints(win)
    fr = _frames(ctx, win, (0, 1, 2), kps)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    free = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, 0.0, -1, opt)
    got = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, 0.0, 3, opt)
    assert got[0].tobytes() == free[0].tobytes() and got[2].tobytes() == free[2].tobytes()
    for t in range(2):
        choked = fr[1 + t].choked_mask(3)
        xy = free[0][t]
        ix = np.clip(np.floor(xy[:, 0] + np.float32(0.5)), 0, W - 1).astype(int)
        iy = np.clip(np.floor(xy[:, 1] + np.float32(0.5)), 0, H - 1).astype(int)
        want = free[1][t] & (choked[iy, ix] != 0)
        assert np.array_equal(got[1][t], want) and 0 < want.sum() < free[1][t].sum()
    _close(fr)


# ---- 6. refusals ----
def test_refusals_at_stage_level_at_the_setters_and_at_submit(ctx):
    win = 10
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    fr = _frames(ctx, win, (0, 1), _keypoints(win))
    for value in (2, -1):
        with pytest.raises(hip.PolychaseHipError, match="mask_windows"):
            hip.lk_track_window_masked(ctx, fr[0], fr[1:], value, opt=opt)
    _close(fr)
    setters = {"normalize": lambda an, on: an.set_normalize(1 if on else 0),
               "affine": lambda an, on: an.set_affine_refinement(1 if on else 0),
               "search": lambda an, on: an.set_search_radius(24 if on else 0),
               "correlation": lambda an, on: an.set_min_correlation(0.5 if on else 0.0)}
    rgb = [np.ascontiguousarray(np.repeat(_frame(k)[0][:, :, None], 3, axis=2)) for k in (0, 1)]
    for name, setter in setters.items():
        an = hip.Analyzer(ctx, W, H, hip.gftt_options(), opt, ring_frames=4, max_jobs=2)
        for value in (2, -1):
            with pytest.raises(hip.PolychaseHipError, match="mask_windows"):
                an.set_mask_windows(value)
        setter(an, True)
        with pytest.raises(hip.PolychaseHipError, match="mask_windows"):
            an.set_mask_windows(1)
        setter(an, False)
        an.set_mask_windows(1)
        setter(an, True)            # switched on afterwards: the job is refused, before anything is launched
        an.put_frame(1, rgb[0])
        an.put_frame(2, rgb[1], will_detect=False)
        with pytest.raises(hip.PolychaseHipError, match="mask_windows"):
            an.submit(1, [2])
        assert an.pending == 0
        setter(an, False)
        an.submit(1, [2])
        an.collect()
        an.close()


# ---- 7. the analyzer: its rows are the stage-level call's ----
def _rgb(k):
    return np.ascontiguousarray(np.repeat(_frame(k)[0][:, :, None], 3, axis=2))


def _assert_job_is_the_stage_call(ctx, win, fopt, job, result, masks, fb):
    f1, tg = job
    got_f1, kps, _, flows = result
    assert got_f1 == f1 and len(kps) >= 10
    times = {1: 0, 2: 1, 3: 2, 4: 3}
    fr = _frames(ctx, win, [times[f1]] + [times[t] for t in tg], kps, [masks[f1]] + [masks[t] for t in tg])
    stage = hip.lk_track_window_masked(ctx, fr[0], fr[1:], 1, fb, -1, fopt)
    plain = hip.lk_track_fb(ctx, fr[0], fr[1:], fb, fopt)
    for k, t in enumerate(tg):
        idx, xy, err = flows[t]
        sel = np.nonzero(stage[1][k] == 1)[0]
        assert len(sel) >= 5 and np.array_equal(idx, sel.astype(np.uint32)), (f1, t)
        assert np.array_equal(_bits(xy), _bits(stage[0][k][sel])) and np.array_equal(_bits(err), _bits(stage[2][k][sel])), (f1, t)
    _close(fr)
    return int(stage[5].sum()), stage[0].tobytes() != plain[0].tobytes()


def test_analyzer_jobs_hold_the_stage_level_rows_while_the_mask_changes(ctx):
    win = 10
    fopt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    an = hip.Analyzer(ctx, W, H, hip.gftt_options(), fopt, ring_frames=17, max_jobs=3)
    an.set_fb_threshold(FB_THRESHOLD)
    an.set_mask_windows(True)
    masks = {}
    for i, k in enumerate((0, 1, 2, 3)):
        if i == 2:
            an.set_mask(None)                   # frame 3 is put without a mask in force: no weights
            masks[i + 1] = None
        else:
            masks[i + 1] = _frame(k)[1]
            an.set_mask(masks[i + 1])           # ... and the others under the disc of their own time
        an.put_frame(i + 1, _rgb(k))
    jobs = ((1, [2, 3]), (2, [3, 4]), (3, [4]))
    for f1, tg in jobs:
        an.submit(f1, tg)
    out = [an.collect() for _ in jobs]
    an.close()
    seen = [_assert_job_is_the_stage_call(ctx, win, fopt, job, res, masks, FB_THRESHOLD) for job, res in zip(jobs, out)]
    assert seen[0][0] >= 3 and seen[1][0] >= 3 and seen[0][1] and seen[1][1], "keypoints detected under the disc lie near its outline too"
    assert seen[2][0] == 0, "frame 3 has no weights"


def test_analyzer_frames_put_without_detection_take_the_mask_and_their_weights(ctx):
    win = 10
    fopt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    an = hip.Analyzer(ctx, W, H, hip.gftt_options(), fopt, ring_frames=17, max_jobs=2)
    an.set_mask_windows(True)
    kps = _keypoints(win)[:55]                  # the caller's keypoints, in the frame
    masks = {}
    for i, k in enumerate((0, 1, 2)):
        masks[i + 1] = _frame(k)[1]
        an.set_mask(masks[i + 1])
        an.put_frame(i + 1, _rgb(k), will_detect=False)
    an.set_keypoints(1, kps)
    an.set_fb_threshold(FB_THRESHOLD)
    an.submit(1, [2, 3])
    res = an.collect()
    an.close()
    assert np.array_equal(res[1], kps)
    touched, moved = _assert_job_is_the_stage_call(ctx, win, fopt, (1, [2, 3]), res, masks, FB_THRESHOLD)
    assert touched >= 30 and moved
