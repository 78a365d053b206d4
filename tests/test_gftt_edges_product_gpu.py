"""GPU: the detection chain's host-side edges through the pipelined analyzer (tests/gftt_dot_scenes.py has the clips,
tests/test_gftt_edges_cpu.py their conditions).  Keypoints AND every flow record are compared with the reference-shaped CPU
path byte for byte; Context.detection_paths() tells which detections were redone.

  hint edge    the launch hint is max(4096, 1.25 x the last finished frame's candidates): a frame with exactly 4096 candidates
               behind frames of 64 fits its launches, one with 4097 raises overflow bit 4 and is redone -- its flow rows depend
               on the keypoints' event being recorded again after the redo
  bucket edge  frames with a value bucket of 512 and of 513 keys in turns: every other frame is redone, with the next frames'
               detections already queued behind it
  table swap   a stage-level detection with another min_distance between an analyzer's put_frame and submit replaces the
               context's cached suppression table under queued work"""
import numpy as np
import pytest

import gftt_dot_scenes as S
import oracle
from polychase_amd import hip
from polychase_amd.pipeline import LOOKAHEAD, ClipAnalyzer

pytestmark = pytest.mark.gpu

REDO = [n for n in hip.DETECT_PATH_NAMES if n.startswith("redo_")]


def _compare_clip(kps_o, flows_o, got_kps, got_flows):
    assert sorted(got_kps) == sorted(kps_o)
    for f in kps_o:
        assert np.array_equal(got_kps[f], kps_o[f]), f"keypoints of frame {f}"
    assert sorted(got_flows) == sorted(flows_o)
    for key in flows_o:
        for a, b in zip(got_flows[key], flows_o[key]):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"flow {key}"


def _run_clip(grays, gftt_kw, between=None):
    """the clip through ClipAnalyzer on a context of its own (the launch hint belongs to the context) and through the CPU path;
    between(ctx), if given, runs after the first frames are put and before any of them is submitted.
    -> (detection_paths, number of flow rows compared)"""
    frames = [S.rgb_of(g) for g in grays]
    h, w = grays[0].shape
    n = len(frames)
    kps_o, flows_o = oracle.analyze_clip(frames, first_frame=1, gopt=oracle.gftt_options(**gftt_kw), fopt=oracle.flow_options(**S.CLIP_FLOW),
                                         threads=4)
    got_kps, got_flows = {}, {}

    def sink(f1, kps, detected, flows):
        assert detected
        got_kps[f1] = kps
        for f2, rec in flows.items():
            got_flows[(f1, f2)] = rec

    ctx = hip.Context(0)
    try:
        an = ClipAnalyzer(ctx, w, h, 1, n, lambda fid: frames[fid - 1], hip.gftt_options(**gftt_kw), hip.flow_options(**S.CLIP_FLOW))
        try:
            ctx.detection_paths(reset=True)
            if between:
                an._ensure_resident(1 + 8 + LOOKAHEAD, 1)      # what submit(1) does first: ten frames put, their detections queued
                between(ctx)
                stage = ctx.detection_paths(reset=True)
                assert stage["finished"] == stage["fast_path"] > 0, stage
            an.run(range(1, n + 1), sink)
            paths = ctx.detection_paths()
        finally:
            an.close()
    finally:
        ctx.close()
    _compare_clip(kps_o, flows_o, got_kps, got_flows)
    rows = sum(len(v[0]) for v in flows_o.values())
    assert rows > 1000, "the clip must have flow rows to compare"
    return paths, rows


@pytest.mark.parametrize("run", list(S.HINT_RUNS))
def test_frame_of_4096_candidates_fits_the_launch_hint(run):
    paths, _ = _run_clip(S.hint_clip(4096), S.HINT_RUNS[run])
    print(paths)
    assert paths["finished"] == paths["fast_path"] == S.HINT_LEAD + S.HINT_EDGE_FRAMES and not any(paths[r] for r in REDO), paths


@pytest.mark.parametrize("run", list(S.HINT_RUNS))
def test_frame_of_4097_candidates_is_redone_for_the_launch_hint(run):
    paths, _ = _run_clip(S.hint_clip(4097), S.HINT_RUNS[run])
    print(paths)
    assert paths["finished"] == S.HINT_LEAD + S.HINT_EDGE_FRAMES
    assert 1 <= paths["redo_overflow_4"] < paths["finished"], "at least one frame is redone for overflow bit 4, and not every frame"
    assert paths["fast_path"] == paths["finished"] - paths["redo_overflow_4"]
    assert not any(paths[r] for r in REDO if r != "redo_overflow_4"), paths
    # the frames of 64 dots fit; every frame of 4097 was queued while the hint stood at 4096
    assert paths["redo_overflow_4"] == S.HINT_EDGE_FRAMES


def test_alternating_bucket_512_and_513_frames():
    paths, _ = _run_clip(S.bucket_clip(), S.BUCKET_CLIP_GFTT)
    print(paths)
    assert paths["finished"] == 12 and paths["redo_overflow_1"] == 6 and paths["fast_path"] == 6, paths
    assert not any(paths[r] for r in REDO if r != "redo_overflow_1"), paths


def _stage_detection_with_radius_3(ctx):
    """a stage-level detection of the tie scene with min_distance 3 (the analyzer's is 7), against the oracle"""
    sc = S.scene("ties_500_w156")
    kw = dict(min_distance=3.0, **S.ONE_CELL)
    want = oracle.gftt(sc.gray, oracle.gftt_options(**kw))
    other = oracle.gftt(sc.gray, oracle.gftt_options(**dict(kw, min_distance=7.0)))
    assert len(want) == 500 and len(other) == 250, "the two radii give different keypoints"
    f = hip.Frame(ctx, sc.w, sc.h, 5, 0)
    try:
        f.set_gray(np.ascontiguousarray(sc.gray))
        f.detect(hip.gftt_options(**kw))
        assert np.array_equal(f.keypoints(), want), "stage-level detection between put_frame and submit"
    finally:
        f.close()


def test_table_swap_under_queued_detections():
    paths, _ = _run_clip(S.ties_clip(), dict(min_distance=7.0, **S.ONE_CELL), between=_stage_detection_with_radius_3)
    assert paths["finished"] == paths["fast_path"] == 12, paths


def test_table_swap_under_queued_detections_that_are_redone():
    """... and with frames among the queued ones that overflow a value bucket.  The clip opens with one: its redo is the first
    thing the analyzer does after the stage call replaced the table (a later put_frame brings the analyzer's table back)"""
    paths, _ = _run_clip(S.bucket_clip(first=513), dict(min_distance=7.0, **S.BUCKET_CLIP_GFTT), between=_stage_detection_with_radius_3)
    assert paths["finished"] == 12 and paths["redo_overflow_1"] == 6 and paths["fast_path"] == 6, paths
