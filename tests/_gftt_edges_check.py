#!/usr/bin/env python3
"""Case list and runner of tests/test_gftt_edges_gpu.py: every scene x option set of tests/gftt_dot_scenes.py through
hip.Frame.detect against the CPU oracle -- the response map bit for bit, the candidate count, the keypoint count, the keypoints
in value and order -- and, from Context.detection_paths(), the path each scene was built for: a scene made to fit must finish
on the fast path (a quiet redo on the slow path would give the right keypoints too), a scene made to overflow must be redone
for that reason and no other.

A case runs on one Frame: first another image of the same size (a sibling scene where the table below names one -- so
bucket_512 follows a frame that overflowed --, else the scene mirrored left to right: as many candidates, elsewhere), then the
scene twice.  State bytes, bucket slots and look-back words left by the previous detection must not show.

The test file runs the cases in its own process (the fused chain for the default response with a table radius) and, through
main() below, once more in a child process under POLYCHASE_GFTT_GENERAL=1 (scatter + bucket sort + suppress_sorted +
accepted_scatter for the same options) and once under POLYCHASE_GFTT_SLOW_PATH=1 (every detection redone: rocPRIM sort, counts
on the host) -- switches the library reads once per process.  One line per case: "PASS <name>" or "FAIL <name> <why>"."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gftt_dot_scenes as S  # noqa: E402
from polychase_amd import hip  # noqa: E402

# the image detected before the scene on the same Frame (same size); None: the scene mirrored
PREVIOUS = {"bucket_512": "bucket_513", "bucket_513": "bucket_512", "bucket_513_masked": "bucket_513",
            "count_1": "count_257", "count_255": "count_257", "count_256": "count_1", "count_257": "count_256",
            "keypoints_4095": "keypoints_4097", "keypoints_4096": "keypoints_4095", "keypoints_4097": "keypoints_4096",
            # 7167 and 7168 leave the frame's keypoint buffer as it was; 7169, once redone, grow it
            "keypoint_capacity_7167": "keypoint_capacity_7168", "keypoint_capacity_7168": "keypoint_capacity_7167",
            "keypoint_capacity_7169": "keypoint_capacity_7167"}
REDO_BOUND_S = 0.1       # tests/test_fused_chain_gpu.py: a suppression that waited for an unowned candidate sits out the tripwire


def case_names():
    return ["%s-%s" % c for c in S.cases()]


def mode_of_process():
    if os.environ.get("POLYCHASE_GFTT_SLOW_PATH") is not None:
        return "slow"
    return "general" if os.environ.get("POLYCHASE_GFTT_GENERAL") == "1" else "default"


def frame_keypoint_capacity(w, h):
    """the keypoint buffer of a stage-level frame (pc_frame_create: room for max(4096, w h / 16), grown by half + 1024)"""
    n = max(4096, w * h // 16)
    return n + n // 2 + 1024


def previous_image(name):
    """-> (gray, mask) of the image a case detects first"""
    if name in PREVIOUS:
        prev = S.scene(PREVIOUS[name])
        return np.ascontiguousarray(prev.gray), prev.mask
    return np.ascontiguousarray(S.scene(name).gray[:, ::-1]), None


def _oracle_counts(name, gray, mask, run):
    """-> (candidates, keypoints, largest value bucket) of an image under the run's options, from the oracle"""
    trial = S.Scene("trial", gray, [], {run: S.scene(name).runs[run]}, mask)
    opt = S.options(trial, run)
    if mask is not None:
        xy, _, ncand = S.ref.gftt(gray, opt, mask)
    else:
        xy, _, ncand = S.oracle.gftt(gray, opt, want_eig=True)
    return ncand, len(xy), int(S.histogram(trial, run)[1].max())


def expected_paths(name, run, mode, detections):
    """the counters of Context.detection_paths() after the `detections` detections of the scene that follow the one of
    previous_image() on a fresh Frame.  Restates detect_finish: a detection is redone when a value bucket holds more than 512
    keys, when the keypoint count reaches the frame's capacity (unless max_corners caps it within the capacity) -- the slow path
    then grows the buffer to what the frame needs, by half + 1024 --, and always under POLYCHASE_GFTT_SLOW_PATH"""
    sc = S.scene(name)
    limit = sc.runs[run].get("max_corners", 0)
    cap = frame_keypoint_capacity(sc.w, sc.h)
    want = dict.fromkeys(hip.DETECT_PATH_NAMES, 0)
    want["finished"] = detections
    images = [_oracle_counts(name, *previous_image(name), run)] + [_oracle_counts(name, sc.gray, sc.mask, run)] * detections
    for k, (ncand, nkp, largest_bucket) in enumerate(images):
        reasons = []
        if largest_bucket > S.BUCKET_SLOTS:
            reasons.append("redo_overflow_1")
        if nkp >= cap and not 0 < limit <= cap:
            reasons.append("redo_keypoints")
        if mode == "slow":
            reasons.append("redo_forced")
        if reasons:
            need = min(ncand, limit) if limit > 0 else ncand
            if need > cap:
                cap = need + need // 2 + 1024
        if k == 0:
            continue
        for r in reasons:
            want[r] += 1
        if not reasons:
            want["fast_path"] += 1
    return want


def detect_mismatch(frame, name, run):
    """'' when the frame's latest detection equals the oracle's, else what differs first"""
    xy, eig, ncand = S.expected(name, run)
    got = frame.min_eig()
    if not np.array_equal(got.view(np.uint32), eig.view(np.uint32)):
        ys, xs = np.nonzero(got.view(np.uint32) != eig.view(np.uint32))
        return "response differs at %d pixels (first x=%d y=%d: %r, expected %r)" % (len(xs), xs[0], ys[0], got[ys[0], xs[0]], eig[ys[0], xs[0]])
    if frame.num_candidates != ncand:
        return "%d candidates, expected %d" % (frame.num_candidates, ncand)
    if frame.num_keypoints != len(xy):
        return "%d keypoints, expected %d" % (frame.num_keypoints, len(xy))
    kp = frame.keypoints()
    if not np.array_equal(kp, xy):
        k = int(np.nonzero(np.any(kp != xy, axis=1))[0][0])
        return "keypoint %d of %d is %s, expected %s" % (k, len(xy), kp[k], xy[k])
    return ""


def run_case(ctx, name, run, mode):
    sc = S.scene(name)
    opt = S.options(sc, run, hip)
    frame = hip.Frame(ctx, sc.w, sc.h, 5, 0)
    try:
        prev_gray, prev_mask = previous_image(name)
        frame.set_gray(prev_gray)
        frame.set_mask(prev_mask)
        frame.detect(opt)
        frame.set_gray(np.ascontiguousarray(sc.gray))
        frame.set_mask(sc.mask)
        ctx.detection_paths(reset=True)
        times = []
        for k in range(2):
            t0 = time.perf_counter()
            frame.detect(opt)
            times.append(time.perf_counter() - t0)
            why = detect_mismatch(frame, name, run)
            if why:
                return "detection %d: %s" % (k + 1, why)
        got, want = ctx.detection_paths(), expected_paths(name, run, mode, 2)
        if got != want:
            return "paths %s, expected %s" % ({k: v for k, v in got.items() if v}, {k: v for k, v in want.items() if v})
        if want["redo_overflow_1"] and min(times) >= REDO_BOUND_S:
            return "the redo of an overflowing bucket took %.1f ms" % (min(times) * 1e3)
        return ""
    finally:
        frame.close()


def run_all(ctx, report, mode):
    for name, run in S.cases():
        try:
            why = run_case(ctx, name, run, mode)
        except hip.PolychaseHipError as e:        # e.g. "suppression kernel did not converge": nothing more on this device
            report("%s-%s" % (name, run), "error: %s" % e)
            return
        report("%s-%s" % (name, run), why)


def main():
    mode = mode_of_process()
    assert mode in ("general", "slow"), "this helper is about POLYCHASE_GFTT_GENERAL=1 and POLYCHASE_GFTT_SLOW_PATH=1"
    ctx = hip.Context(0)
    run_all(ctx, lambda name, why: print(("FAIL %s %s" % (name, why)) if why else ("PASS %s" % name), flush=True), mode)
    ctx.close()


if __name__ == "__main__":
    main()
