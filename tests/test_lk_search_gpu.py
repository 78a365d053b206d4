"""GPU: the search prepass at stage level (kernels_lk_search.hip through pc_lk_track_search) against the numpy restatement of the
rule (tests/lk_search_ref.py) applied to the oracle's forward rows, bit for bit, in both arithmetic modes.  The scene is
tests/lk_search_scene.py's: 160 x 120 gray frames, max_level 2, eight targets, 73 keypoints; the reference of a (window, radius,
mode, threshold) is computed once and shared."""
import numpy as np
import pytest

import lk_affine_ref as aff_ref
import lk_search_ref as ref
import lk_search_scene as scene
import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ARITH = {"canonical": (hip.ARITH_CANONICAL, oracle.EMU_CANONICAL), "opencv_x86": (hip.ARITH_OPENCV_X86, oracle.EMU_OPENCV_X86)}
MAX_LEVEL = scene.MAX_LEVEL
NAMES = ("next_xy", "status", "err", "search_d", "search_state", "back_xy", "back_status")
GOT = (0, 1, 2, 7, 8, 3, 4)          # where lk_track_search returns them
FB = 1.0


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_arithmetic(hip.ARITH_CANONICAL)
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _frames(ctx, win, grays=None):
    fr = []
    for g in grays if grays is not None else [scene.frame1()] + scene.targets():
        f = hip.Frame(ctx, scene.W, scene.H, win, MAX_LEVEL)
        f.set_gray(np.array(g))
        fr.append(f)
    fr[0].set_keypoints(np.array(scene.keypoints(), np.float32))
    return fr


def _close(fr):
    for f in fr:
        f.close()


def _assert_same(got, want, name, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, name, got.shape, want.shape, got.dtype, want.dtype)
    d = _bits(got) != _bits(want)
    bad = np.nonzero(d.reshape(len(want), -1).any(axis=1))[0] if len(want) else []
    assert not len(bad), (what, name, "rows", bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())


def _check_reference(win, R, emu):
    """asserted on the REFERENCE, before anything is compared with it"""
    fwd, rows = scene.forward(win, emu), scene.reference(win, R, emu)
    state = np.stack([r[4] for r in rows])
    assert (state == ref.NONE).any() and (state == ref.REPLACED).any() and (state == ref.KEPT).any(), (win, R, np.bincount(state.ravel(), minlength=3))
    rescued = sum(int(((f[1] == 0) & (r[4] == ref.REPLACED)).sum()) for f, r in zip(fwd, rows))
    assert rescued >= 1, (win, R, "no forward status-0 row is rescued")
    assert not state[0].any() and not state[4].any(), "the unchanged and the flat target are not searched into"
    return state


# ---- 1. bit parity of the stage call, without and with the backward pass ----
@pytest.mark.parametrize("arith", sorted(ARITH))
@pytest.mark.parametrize("R", [5, 16, 40, 200])
@pytest.mark.parametrize("win", [3, 10, 21])
def test_stage_call_matches_the_reference_bit_for_bit(ctx, win, R, arith):
    emu = ARITH[arith][1]
    _check_reference(win, R, emu)
    ctx.set_arithmetic(ARITH[arith][0])
    fr = _frames(ctx, win)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    plain = hip.lk_track(ctx, fr[0], fr[1:], opt)
    got = {fb: hip.lk_track_search(ctx, fr[0], fr[1:], R, fb_threshold=fb, opt=opt) for fb in (0.0, FB)}
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    _close(fr)
    fwd = scene.forward(win, emu)
    for t in range(8):
        for k in range(3):      # the forward part is the oracle's in this mode
            _assert_same(plain[k][t], fwd[t][k], "forward " + NAMES[k], (win, R, arith, scene.MIX8[t]))
    for fb in (0.0, FB):
        want = scene.reference(win, R, emu, fb)
        if fb:
            dropped = sum(int(((a[1] == 1) & (b[1] == 0)).sum()) for a, b in zip(scene.reference(win, R, emu), want))
            guided_kept = sum(int(((b[4] == ref.REPLACED) & (b[1] == 1)).sum()) for b in want)
            assert dropped >= 5 and guided_kept >= 5, (win, R, dropped, guided_kept)          # on the reference
        for t in range(8):
            for name, g, w in zip(NAMES, GOT, range(7)):
                _assert_same(got[fb][g][t], want[t][w], name, (win, R, arith, fb, scene.MIX8[t]))
        assert not got[fb][5].any() and not got[fb][6].any(), "no refinement was asked for"


@pytest.mark.parametrize("win", [3, 10, 21])
def test_both_arithmetic_modes_search_alike(win):
    """the search and the guided pass take no part in the arithmetic mode: d is the same, and a pair replaced in both modes holds
    the same record (a pair's state may differ, since it is decided against the mode's own forward error)"""
    R = 40
    a, b = (scene.reference(win, R, ARITH[m][1]) for m in sorted(ARITH))
    both = 0
    for ra, rb in zip(a, b):
        assert np.array_equal(ra[3], rb[3])
        sel = (ra[4] == ref.REPLACED) & (rb[4] == ref.REPLACED)
        both += int(sel.sum())
        assert ra[0][sel].tobytes() == rb[0][sel].tobytes() and ra[2][sel].tobytes() == rb[2][sel].tobytes()
    assert both >= 10


# ---- 2. option off ----
def test_radius_0_gives_the_bytes_of_the_affine_call_and_launches_nothing_new(ctx):
    win = 10
    fr = _frames(ctx, win)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    for affine, normalize, thr, fb in ((0, 0, 0.0, 0.0), (1, 0, 0.75, FB), (0, 1, 0.75, FB), (0, 0, 0.0, FB)):
        want = hip.lk_track_affine(ctx, fr[0], fr[1:], affine, normalize, thr, fb, -1, opt)
        off = hip.lk_track_search(ctx, fr[0], fr[1:], 0, affine, normalize, thr, fb, -1, opt)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(off[:7], want)), (affine, normalize, thr, fb)
        assert not off[7].any() and not off[8].any()
    ctx.enable_timing(True)
    counts = []
    for call in (lambda: hip.lk_track_affine(ctx, fr[0], fr[1:], 0, 0, 0.75, FB, -1, opt),
                 lambda: hip.lk_track_search(ctx, fr[0], fr[1:], 0, 0, 0, 0.75, FB, -1, opt),
                 lambda: hip.lk_track_search(ctx, fr[0], fr[1:], 40, 0, 0, 0.75, FB, -1, opt)):
        ctx.reset_timing()
        call()
        counts.append({k: v[0] for k, v in ctx.timing().items()})
    ctx.enable_timing(False)
    _close(fr)
    assert counts[0] == counts[1], counts
    # the search is timed under the forward launch's class, the backward pass of its rows under the backward launch's
    assert counts[2] == {**counts[0], "lk": 2, "lk_fb": 2}, counts
    assert counts[0]["lk"] == 1 and counts[0]["lk_fb"] == 1 and counts[0]["lk_corr"] == 1, counts


# ---- 3. the forward-backward check: untouched rows are judged as without the option ----
@pytest.mark.parametrize("arith", sorted(ARITH))
def test_forward_backward_status_of_untouched_rows_equals_the_option_off_run(ctx, arith):
    win, R = 10, 40
    ctx.set_arithmetic(ARITH[arith][0])
    fr = _frames(ctx, win)
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    off = hip.lk_track_search(ctx, fr[0], fr[1:], 0, fb_threshold=FB, opt=opt)
    on = hip.lk_track_search(ctx, fr[0], fr[1:], R, fb_threshold=FB, opt=opt)
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    _close(fr)
    state = on[8]
    same = state != ref.REPLACED
    assert same.sum() >= 100 and (state == ref.KEPT).sum() >= 10 and (off[1][same] == 1).sum() >= 50
    for k in range(5):
        assert on[k][same].tobytes() == off[k][same].tobytes(), NAMES[k]
    want = scene.reference(win, R, ARITH[arith][1], FB)
    rep = ~same
    assert rep.sum() >= 20
    for t in range(8):
        for k, w in ((1, 1), (3, 5), (4, 6)):
            assert on[k][t][rep[t]].tobytes() == want[t][w][rep[t]].tobytes(), (k, t)


# ---- 4. the refinement judges the chosen end points ----
def test_affine_refinement_runs_on_the_searched_records(ctx):
    win, R = 10, 40
    rows = scene.reference(win, R, oracle.EMU_CANONICAL)
    p1, pts = scene.pyramids(win)
    oopt = oracle.flow_options(window_size=win, max_level=MAX_LEVEL)
    want = aff_ref.refine(aff_ref.Planes(p1), [aff_ref.Planes(p) for p in pts], scene.keypoints(), [r[:3] for r in rows], oopt)
    moved = sum(int(((w[4] == aff_ref.ACCEPTED) & (r[4] == ref.REPLACED)).sum()) for w, r in zip(want, rows))
    assert moved >= 10, "rows the search replaced are refined"          # on the reference
    ctx.set_arithmetic(hip.ARITH_CANONICAL)
    fr = _frames(ctx, win)
    got = hip.lk_track_search(ctx, fr[0], fr[1:], R, 1, opt=hip.flow_options(window_size=win, max_level=MAX_LEVEL))
    _close(fr)
    for t in range(8):
        for g, w, name in ((0, 0, "next_xy"), (1, 1, "status"), (2, 2, "err"), (5, 3, "affine_m"), (6, 4, "affine_state")):
            _assert_same(got[g][t], want[t][w], name, scene.MIX8[t])
        _assert_same(got[7][t], rows[t][3], "search_d", scene.MIX8[t])
        _assert_same(got[8][t], rows[t][4], "search_state", scene.MIX8[t])


# ---- 5. arguments ----
def test_a_radius_out_of_range_and_the_combination_with_normalize_are_refused_before_anything_is_launched(ctx):
    win = 10
    fr = _frames(ctx, win, [scene.frame1(), scene.target((19, -11))])
    opt = hip.flow_options(window_size=win, max_level=MAX_LEVEL)
    ctx.enable_timing(True)
    ctx.reset_timing()
    for value in (-1, 257):
        with pytest.raises(hip.PolychaseHipError, match="search_radius"):
            hip.lk_track_search(ctx, fr[0], fr[1:], value, opt=opt)
    with pytest.raises(hip.PolychaseHipError, match="normalize"):
        hip.lk_track_search(ctx, fr[0], fr[1:], 64, 0, 1, opt=opt)
    launched = {k: v[0] for k, v in ctx.timing().items() if v[0]}
    ctx.enable_timing(False)
    assert not launched, launched
    hip.lk_track_search(ctx, fr[0], fr[1:], 256, opt=opt)
    hip.lk_track_search(ctx, fr[0], fr[1:], 1, opt=opt)
    an = hip.Analyzer(ctx, scene.W, scene.H, hip.gftt_options(), opt)
    for value in (-1, 257):
        with pytest.raises(hip.PolychaseHipError, match="search_radius"):
            an.set_search_radius(value)
    an.set_normalize(1)
    with pytest.raises(hip.PolychaseHipError, match="normalize"):
        an.set_search_radius(64)
    an.set_normalize(0)
    an.set_search_radius(64)
    an.set_normalize(1)          # switched on behind the search: the job is refused
    frames = scene.clip(2)
    an.put_frame(1, frames[0])
    an.put_frame(2, frames[1])
    with pytest.raises(hip.PolychaseHipError, match="normalize"):
        an.submit(1, [2])
    an.close()
    _close(fr)
