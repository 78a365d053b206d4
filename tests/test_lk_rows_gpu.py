"""GPU: the small kernels every flow row passes through (kernels_lk.hip: bin_count / bin_scan / bin_scatter, compact_count with the
scan in its tail, compact_scatter, unpack_records, copy_keypoints) at DICTATED status patterns -- the cases of
tests/lk_rows_cases.py, whose coverage tests/test_lk_rows_cpu.py asserts.  Everything is compared bit for bit.

  stage calls      pc_lk_track_masked under margin 0 returns the dictated pattern, and next_xy / status / err are oracle.lk filtered
                   by target_mask_ref.keep, in canonical arithmetic and in the x86 order: unpack_records_kernel and slot_of, without
                   the compaction.  (An out-of-frame row has status 0 and err 0; its next_xy is compared nowhere in the suite --
                   tests/lk_subpixel_scene.mismatch -- and is not here.)
  filtered calls   pc_lk_track_filtered / _filtered_fb = rows() of pc_lk_track / _fb, on ONE context in an order that shrinks and
                   grows n and n_targets, so the lane's tickets and scratch are reused
  analyzer         per case, the collected job = rows() of the stage call and the keypoints come back as supplied; then sequences of
                   fourteen jobs per analyzer that reuse each lane with fewer targets, fewer blocks, no keypoint and no target,
                   every second one with a device log
  bin-scan edges   256 and 272 tiles through pc_lk_track against the oracle and through pc_lk_track_filtered against rows()

Cases kept for what they caught go to the end of K.TABLE under a comment that names it; none so far."""
import numpy as np
import pytest

import lk_rows_cases as K
from polychase_amd import hip

pytestmark = pytest.mark.gpu

ARITH = {"canonical": hip.ARITH_CANONICAL, "x86": hip.ARITH_OPENCV_X86}
# forward-backward threshold of the _fb calls: the median distance between a keypoint and its row tracked back, on the CPU oracle
# (0.00051 .. 0.00057 px per target on these frames, both windows), so about half of the rows pass: an irregular pattern that is
# not dictated; rows() of pc_lk_track_fb's own status is the reference for it
FB = 0.0005


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.set_arithmetic(hip.ARITH_CANONICAL)
    c.close()


@pytest.fixture
def arith(ctx, request):
    """the context in the arithmetic mode named by the test's `mode` parameter, canonical again afterwards"""
    ctx.set_arithmetic(ARITH[request.node.callspec.params["mode"]])
    yield ctx
    ctx.set_arithmetic(hip.ARITH_CANONICAL)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _frames(ctx, c):
    fr = []
    for k, g in enumerate(c.grays):
        f = hip.Frame(ctx, c.w, c.h, c.win, K.MAX_LEVEL)
        f.set_gray(np.array(g))
        if k > 0 and c.masks[k - 1] is not None:
            f.set_mask(np.array(c.masks[k - 1]))
        fr.append(f)
    fr[0].set_keypoints(np.array(c.kps))
    return fr


def _opt(c):
    return hip.flow_options(window_size=c.win, max_level=K.MAX_LEVEL)


def _masked_stage_call(ctx, c):
    fr = _frames(ctx, c)
    got = hip.lk_track_masked(ctx, fr[0], fr[1:], 0.0, 0, _opt(c))
    for f in fr:
        f.close()
    return got


def _assert_rows(got, want, what):
    """got: per target (idx, xy, err) as the filtered calls and Analyzer.collect give them; want: K.rows(..)"""
    want = K.split_rows(want)
    assert len(got) == len(want), (what, len(got), len(want))
    for t, ((gi, gx, ge), (wi, wx, we)) in enumerate(zip(got, want)):
        assert gi.dtype == np.uint32 and len(gi) == len(wi), (what, "target", t, "rows", len(gi), len(wi))
        assert gi.tobytes() == wi.tobytes(), (what, "target", t, "src_indices", np.nonzero(gi != wi)[0][:8].tolist())
        assert gx.tobytes() == wx.tobytes(), (what, "target", t, "tgt_xy", np.nonzero((_bits(gx) != _bits(wx)).any(axis=1))[0][:8].tolist())
        assert ge.tobytes() == we.tobytes(), (what, "target", t, "err", np.nonzero(_bits(ge) != _bits(we))[0][:8].tolist())


def _assert_stage(c, got, ref, what, masked=True):
    xy, st, err = got
    oxy, ost, oerr, kept = ref
    want_st = kept if masked else ost
    assert xy.shape == oxy.shape and st.shape == ost.shape and err.shape == oerr.shape and st.dtype == np.uint8, what
    ok = ~c.far
    for t in range(c.n_targets):
        bad = np.nonzero(st[t] != want_st[t])[0]
        assert not len(bad), (what, "target", t, "status at", bad[:8].tolist(), st[t][bad[:8]].tolist())
        bad = np.nonzero((_bits(xy[t]) != _bits(oxy[t])).any(axis=1) & ok)[0]
        assert not len(bad), (what, "target", t, "next_xy at", bad[:8].tolist(), xy[t][bad[:2]].tolist(), oxy[t][bad[:2]].tolist())
        bad = np.nonzero(_bits(err[t]) != _bits(oerr[t]))[0]
        assert not len(bad), (what, "target", t, "err at", bad[:8].tolist(), err[t][bad[:2]].tolist(), oerr[t][bad[:2]].tolist())


# ---- stage calls ----
@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.NAMES)
def test_masked_stage_call_returns_the_dictated_pattern_and_the_oracle_s_rows(arith, name, mode):
    c = K.case(name)
    ref = K.reference(name, mode)
    got = _masked_stage_call(arith, c)
    want = K.expected_status(c, ref[1])
    for t in range(c.n_targets):
        assert np.array_equal(got[1][t], want[t]), (name, mode, "target", t, "the pattern", np.nonzero(got[1][t] != want[t])[0][:8].tolist())
    _assert_stage(c, got, ref, (name, mode))


# all-ones and out-of-frame cases in the order n 8193 -> 1 -> 257 -> 8193 -> 1 and n_targets 8 -> 1 -> 3 -> 8 -> 1: every call
# after the first finds the tickets and the scratch of ctx->lanes[0] as the call before left them
FILTERED_ORDER = tuple(K.NAMES[k] for k in (22, 2, 12, 23, 0))


@pytest.mark.parametrize("mode", K.MODES)
def test_filtered_stage_calls_give_rows_of_the_raw_calls_while_the_lane_shrinks_and_grows(arith, mode):
    shapes = []
    for name in FILTERED_ORDER:
        c = K.case(name)
        assert c.all_ones, name
        opt = _opt(c)
        fr = _frames(arith, c)
        raw = hip.lk_track(arith, fr[0], fr[1:], opt)
        rows = hip.lk_track_filtered(arith, fr[0], fr[1:], opt)
        raw_fb = hip.lk_track_fb(arith, fr[0], fr[1:], FB, opt)
        rows_fb = hip.lk_track_filtered_fb(arith, fr[0], fr[1:], FB, opt)
        for f in fr:
            f.close()
        _assert_stage(c, raw, K.reference(name, mode), (name, mode, "lk_track"), masked=False)
        assert (raw[1][:, ~c.far] == 1).all() and (raw[1][:, c.far] == 0).all(), (name, mode)
        _assert_rows(rows, K.rows(raw[1], raw[0], raw[2]), (name, mode, "lk_track_filtered"))
        assert raw_fb[0].tobytes() == raw[0].tobytes() and raw_fb[2].tobytes() == raw[2].tobytes(), (name, mode, "the check leaves xy and err")
        _assert_rows(rows_fb, K.rows(raw_fb[1], raw_fb[0], raw_fb[2]), (name, mode, "lk_track_filtered_fb"))
        if c.n >= 257:
            assert all(0.25 * len(r[0]) < len(b[0]) < 0.75 * len(r[0]) for r, b in zip(rows, rows_fb)), (name, mode, "the check keeps about half")
        print(name, mode, "rows per target", [len(r[0]) for r in rows], "after the backward check", [len(r[0]) for r in rows_fb])
        shapes.append((c.n, c.n_targets))
    assert shapes[:4] == [(8193, 8), (1, 1), (257, 3), (8193, 8)]


# ---- analyzer ----
FIRST_TARGET_ID = 16          # frame ids of the targets; a job's frame1 takes 1 + its number: distinct slots of a 32-frame ring
RING = 32


def _put_targets(an, c):
    """the case's targets under ids FIRST_TARGET_ID.., each with its own mask under margin 0, or none under margin -1"""
    for t, m in enumerate(c.masks):
        an.set_mask(None if m is None else np.array(m))
        an.set_target_mask_margin(-1 if m is None else 0)
        an.put_frame(FIRST_TARGET_ID + t, K.rgb(c.grays[1 + t]), will_detect=False)
    an.set_mask(None)
    an.set_target_mask_margin(-1)


def _assert_job(c, result, frame1, stage, what):
    f1, kps, detected, flows = result
    assert f1 == frame1 and not detected, what
    assert kps.dtype == np.float32 and kps.shape == (c.n, 2) and kps.tobytes() == c.kps.tobytes(), (what, "the keypoints come back as supplied")
    ids = [FIRST_TARGET_ID + t for t in range(c.n_targets)]
    assert sorted(flows) == ids, (what, sorted(flows))
    _assert_rows([flows[i] for i in ids], K.rows(stage[1], stage[0], stage[2]), what)


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.NAMES)
def test_analyzer_job_holds_rows_of_the_stage_call_and_the_supplied_keypoints(arith, name, mode):
    c = K.case(name)
    stage = _masked_stage_call(arith, c)
    assert np.array_equal(stage[1], K.expected_status(c, K.reference(name, mode)[1])), (name, mode)
    an = hip.Analyzer(arith, c.w, c.h, hip.gftt_options(), _opt(c), ring_frames=RING, max_jobs=2)
    an.put_frame(1, K.rgb(c.grays[0]), will_detect=False)
    _put_targets(an, c)
    an.set_keypoints(1, np.array(c.kps))
    an.submit(1, [FIRST_TARGET_ID + t for t in range(c.n_targets)])
    result = an.collect()
    an.close()
    _assert_job(c, result, 1, stage, (name, mode))


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("max_jobs", [1, 2, 3])
def test_analyzer_lanes_reused_with_fewer_targets_fewer_blocks_no_keypoint_and_no_target(arith, max_jobs, mode):
    from polychase_amd import distributed as D
    jobs = K.sequence_jobs(max_jobs)
    assert [(c.n, c.n_targets) for c in jobs[0::2]] == list(K.LANE_SEQUENCE) == [(c.n, c.n_targets) for c in jobs[1::2]]
    full = max(jobs, key=lambda c: c.n_targets)
    assert full.n_targets == K.MAX_TARGETS
    an = hip.Analyzer(arith, K.W, K.H, hip.gftt_options(), _opt(full), ring_frames=RING, max_jobs=max_jobs)
    log = None
    if max_jobs % 2 == 1:
        import torch
        log = torch.empty(D.log_capacity_bytes(len(jobs), max(c.n for c in jobs) + 64, K.MAX_TARGETS), dtype=torch.uint8, device="cuda")
        an.set_device_log(log)
    _put_targets(an, full)
    f1 = K.rgb(full.grays[0])
    results = []
    for j, c in enumerate(jobs):
        an.put_frame(1 + j, f1, will_detect=False)
        an.set_keypoints(1 + j, np.array(c.kps))
        if an.pending == max_jobs:
            results.append(an.collect())
        an.submit(1 + j, [FIRST_TARGET_ID + t for t in range(c.n_targets)])
    while an.pending:
        results.append(an.collect())
    recs = None
    if log is not None:
        arith.synchronize()
        recs = D.parse_device_log(log.cpu().numpy(), an.device_log_used)
    an.close()
    assert len(results) == len(jobs)
    for j, (c, result) in enumerate(zip(jobs, results)):
        what = ("max_jobs", max_jobs, mode, "job", j, "lane", j & 1, "n", c.n, "targets", c.n_targets)
        if c.n_targets:
            stage = _masked_stage_call(arith, c)
            assert np.array_equal(stage[1], c.want.astype(np.uint8)), (what, "the pattern")
        else:
            stage = (np.zeros((0, c.n, 2), np.float32), np.zeros((0, c.n), np.uint8), np.zeros((0, c.n), np.float32))
        _assert_job(c, result, 1 + j, stage, what)
    print("max_jobs", max_jobs, mode, "rows per job", [sum(len(v[0]) for v in r[3].values()) for r in results], "device log", recs is not None)
    if recs is not None:
        (ha, pa), (hb, pb) = D.pack_records([(r[0], r[1], r[3]) for r in results]), D.pack_records(recs)
        assert np.array_equal(ha, hb) and np.array_equal(pa, pb), "the device log holds the host's records"


# ---- the edges of bin_scan_kernel ----
@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", K.GEOMETRY_NAMES)
def test_bin_scan_at_one_and_two_tiles_per_lane(arith, name, mode):
    c = K.case(name)
    opt = _opt(c)
    fr = _frames(arith, c)
    raw = hip.lk_track(arith, fr[0], fr[1:], opt)
    rows = hip.lk_track_filtered(arith, fr[0], fr[1:], opt)
    for f in fr:
        f.close()
    _assert_stage(c, raw, K.reference(name, mode), (name, mode, "lk_track"), masked=False)
    assert (raw[1] == 1).all(), (name, mode)
    _assert_rows(rows, K.rows(raw[1], raw[0], raw[2]), (name, mode, "lk_track_filtered"))
