"""GPU: the passes behind the forward LK launch at random frame geometries -- the seeded cases of tests/lk_passes_cases.py through
the stage call of their family (pc_lk_track_search, pc_lk_track_normalized, pc_lk_track_window_masked), every returned array
against the chained numpy restatements (lk_passes_cases.reference), bit for bit, in canonical arithmetic and in the x86 order; then
random clips of the same geometries through the analyzer, whose jobs must hold the status-1 rows of that stage call.

What the list covers is asserted on the reference alone in tests/test_lk_passes_random_cpu.py."""
import numpy as np
import pytest

import lk_passes_cases as K
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ARITH = {"canonical": hip.ARITH_CANONICAL, "x86": hip.ARITH_OPENCV_X86}
# the arrays a family's stage call returns, in its order
RETURNS = {"constancy": ("next_xy", "status", "err", "back_xy", "back_status", "affine_m", "affine_state", "search_d", "search_state"),
           "normalized": ("next_xy", "status", "err", "back_xy", "back_status"),
           "window_masked": ("next_xy", "status", "err", "back_xy", "back_status", "touched")}
# Seeds kept for what they caught go here, under a comment that names it; none so far.
SEEDS = tuple(K.SEEDS)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_arithmetic(hip.ARITH_CANONICAL)
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _assert_same(got, want, name, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, name, got.shape, want.shape, got.dtype, want.dtype)
    if name == "touched":
        got, want = got[None], want[None]
    for t in range(len(want) if want.size else 0):      # (no keypoint: the shapes are all there is to compare)
        d =(_bits(got[t]) != _bits(want[t])).reshape(want.shape[1], -1).any(axis=1)
        bad = np.nonzero(d)[0]
        assert not len(bad), (what, name, "target", t, "rows", bad[:8].tolist(), got[t][bad[:2]].tolist(), want[t][bad[:2]].tolist())


def stage_call(ctx, c, frame1, targets, opt):
    """the stage call of the case's family under the case's options -> {name: array}"""
    if c.family == "constancy":
        out = hip.lk_track_search(ctx, frame1, targets, c.R, c.affine, 0, c.min_correlation, c.fb, c.margin, opt)
    elif c.family == "normalized":
        out = hip.lk_track_normalized(ctx, frame1, targets, 1, c.min_correlation, c.fb, c.margin, opt)
    else:
        out = hip.lk_track_window_masked(ctx, frame1, targets, 1, c.fb, c.margin, opt)
    return dict(zip(RETURNS[c.family], out))


def _frames(ctx, c, images, masks, kps, rgb=False):
    fr = []
    for img, m in zip(images, masks):
        f = hip.Frame(ctx, c.w, c.h, c.win, c.max_level)
        (f.set_rgb if rgb else f.set_gray)(np.array(img))
        if m is not None:
            f.set_mask(np.array(m))
        fr.append(f)
    fr[0].set_keypoints(np.array(kps, np.float32).reshape(-1, 2))
    return fr


def check_seed(ctx, seed):
    """one seeded case in both arithmetic modes (tests/soak_parity.py --passes runs this over any seed range)"""
    c = K.case(seed)
    opt = hip.flow_options(**c.flow_kw())
    for mode in K.MODES:
        want = K.reference(c, mode)
        ctx.set_arithmetic(ARITH[mode])
        try:
            fr = _frames(ctx, c, c.grays, c.masks, c.kps)
            assert fr[0].num_levels == c.T + 1, (c.describe(), fr[0].num_levels)
            got = stage_call(ctx, c, fr[0], fr[1:], opt)
            for f in fr:
                f.close()
        finally:
            ctx.set_arithmetic(hip.ARITH_CANONICAL)
        for name in RETURNS[c.family]:
            _assert_same(got[name], want[name], name, (c.describe(), mode))


@pytest.mark.parametrize("seed", SEEDS)
def test_stage_call_matches_the_chained_restatements_bit_for_bit(ctx, seed):
    check_seed(ctx, seed)


# ---- random clips through the analyzer ----
def _configure(an, c):
    if c.family == "constancy":
        an.set_search_radius(c.R)
        an.set_affine_refinement(c.affine)
    elif c.family == "normalized":
        an.set_normalize(1)
    else:
        an.set_mask_windows(True)
    if c.family != "window_masked":
        an.set_min_correlation(c.min_correlation)
    an.set_fb_threshold(c.fb)
    an.set_target_mask_margin(c.margin)


@pytest.mark.parametrize("k", range(len(K.CLIP_SEEDS)))
def test_analyzer_jobs_hold_the_status_1_rows_of_the_stage_call(ctx, k):
    from polychase_amd import distributed as D
    clip = K.clip(k)
    c = clip.case
    opt = hip.flow_options(**c.flow_kw())
    nf = len(clip.rgb)
    assert clip.ring < nf, "frames are evicted during the clip"
    an = hip.Analyzer(ctx, c.w, c.h, hip.gftt_options(max_corners=clip.max_corners), opt, ring_frames=clip.ring, max_jobs=clip.max_jobs)
    _configure(an, c)
    log = None
    if clip.log:
        import torch
        log = torch.empty(D.log_capacity_bytes(nf, max(clip.counts) + 64, clip.ring), dtype=torch.uint8, device="cuda")
        an.set_device_log(log)
    results, put = [], -1
    for f1, tg in clip.jobs:
        upto = min(f1 - clip.first + 1, nf - 1)
        while put < upto:           # ... which evicts frame put + 1 - ring while the jobs before this one may still read it
            put += 1
            an.set_mask(None if clip.masks[put] is None else np.array(clip.masks[put]))
            an.put_frame(clip.first + put, np.array(clip.rgb[put]))
        if an.pending == clip.max_jobs:
            results.append(an.collect())
        an.submit(f1, tg)
    while an.pending:
        results.append(an.collect())
    recs = None
    if log is not None:
        ctx.synchronize()
        used = an.device_log_used
        recs = D.parse_device_log(log.cpu().numpy(), used)
    an.close()
    assert [r[0] for r in results] == [j[0] for j in clip.jobs] and all(r[2] for r in results), "every job, in order, on detected keypoints"
    counts = [len(r[1]) for r in results]
    print(c.describe(), "| frames", nf, "ring", clip.ring, "max_jobs", clip.max_jobs, "max_corners", clip.max_corners, "keypoints", counts)
    assert len(set(counts)) > 1, counts
    # job j runs on lane j & 1: some job holds more keypoints than every job before it on its lane, whose buffers then grow
    assert any(j >= 2 and counts[j] > max(counts[j % 2:j:2]) for j in range(nf)), counts
    rows = 0
    for (f1, tg), (_, kps, _, flows) in zip(clip.jobs, results):
        assert sorted(flows) == sorted(tg)
        ids = [f1 - clip.first] + [t - clip.first for t in tg]
        fr = _frames(ctx, c, [clip.rgb[i] for i in ids], [clip.masks[i] for i in ids], kps, rgb=True)
        stage = stage_call(ctx, c, fr[0], fr[1:], opt)
        for f in fr:
            f.close()
        for t, tid in enumerate(tg):
            keep = np.nonzero(stage["status"][t] == 1)[0].astype(np.uint32)
            idx, xy, err = flows[tid]
            what = (c.describe(), "job", f1, "target", tid)
            assert idx.dtype == np.uint32 and idx.tobytes() == keep.tobytes(), (what, "src_indices", len(idx), len(keep))
            assert xy.tobytes() == stage["next_xy"][t][keep].tobytes(), (what, "tgt_xy")
            assert err.tobytes() == stage["err"][t][keep].tobytes(), (what, "err")
            rows += len(keep)
    assert rows >= 1
    if recs is not None:
        host = [(r[0], r[1], r[3]) for r in results]
        (ha, pa), (hb, pb) = D.pack_records(host), D.pack_records(recs)
        assert np.array_equal(ha, hb) and np.array_equal(pa, pb), "the device log holds the host's records"
