#!/usr/bin/env python3
"""lk_bench.py -- the pyramidal LK launch alone (run ON the GPU box).

One interior frame1 of the synthetic clip and its 8 targets are made resident through the stage-level
C ABI, then `pc_lk_track` is repeated: the LK class is timed with HIP events by the library
(pc_context_enable_timing), launches do not overlap, nothing else runs.  Prints one JSON line with
the average launch time and a checksum of the raw outputs (equal checksums <=> bit-identical
results, the way kernel variants are compared: POLYCHASE_HIP_LIB selects the library).

    python tools/lk_bench.py [--config c2|c3] [--reps 20] [--fb PX] [--min-correlation V] [--normalize] [--affine] [--search-radius N]
                             [--mask-fraction F] [--mask-windows]

--fb PX also times the forward-backward check (pc_lk_track_fb, threshold PX): the forward launch and the backward launch of
the same call, and as the baseline the same backward work through the calls that existed before it -- per target,
set_keypoints(q[status_f == 1]) on the target frame and pc_lk_track(target, [frame1]): eight launches.
--min-correlation V also times the minimum-correlation check (pc_lk_track_correlated, threshold V): the forward launch and the
correlation launch of the same call, and the share of rows the check drops.
--normalize also times the brightness-normalised launch (pc_lk_track_normalized, normalize = 1) and reports its ratio to the plain
launch measured above; with --fb PX the normalised backward launch beside it, against the plain backward launch.
--affine also times the affine refinement (pc_lk_track_affine, affine = 1): its launch is timed under the forward launch's class, so
the figure is the class total of the calls with the option minus that of the same number of calls without it.
--search-radius N also times the search prepass (pc_lk_track_search, search_radius = N), the same way as --affine; --shift DX DY
tracks into targets that are frame1 shifted by whole pixels (k * DX / 8, k * DY / 8 for the k-th skip), where the search has work.
--mask-fraction F puts frame1 and the targets under a polygon mask (an ellipse-like 32-gon over the fraction F of the frame) before
frame1 is detected, so the keypoints lie inside it; --mask-windows then also times the masked windows (pc_lk_track_window_masked):
the masked launch is timed under the forward launch's class, so its figure is the class total of the calls with the option minus
that of the calls without it, in alternating rounds; with --fb PX the weighted backward launch beside the plain one.

(Parity against the CPU oracle is the test suite's business: tests/test_gpu_parity.py, tests/test_fullsize_gpu.py.)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c1": (640, 480, 3), "c2": (1920, 1080, 3), "c3": (3840, 2160, 4)}
SKIPS = (-8, -4, -2, -1, 1, 2, 4, 8)


def fb_timing(ctx, hip, f1, targets, fopt, thr, reps, xy, st, err):
    """forward + backward launch of pc_lk_track_fb against the eight-launch composition; the two must agree bit for bit.
    Call it last: the composition leaves the forward end points as the target frames' keypoints."""
    kps = f1.keypoints()
    res = hip.lk_track_fb(ctx, f1, targets, thr, fopt)      # warm-up + the output that is compared
    fxy, fst, ferr, bxy, bst = res
    assert np.array_equal(fxy, xy) and np.array_equal(ferr, err), "the check changed a forward value"
    ctx.enable_timing(["lk", "lk_fb"])
    ctx.reset_timing()
    for _ in range(reps):
        hip.lk_track_fb(ctx, f1, targets, thr, fopt)
    t = ctx.timing()
    fwd_ms, back_ms = t["lk"][1] / max(1, t["lk"][0]), t["lk_fb"][1] / max(1, t["lk_fb"][0])
    # the composition: every target's surviving end points become ITS keypoints, tracked into frame1 by the forward kernel
    thr2 = np.float32(np.float64(thr) * np.float64(thr))
    comp_ms, agree = 0.0, True
    for rep in range(reps + 1):
        ctx.reset_timing()
        for k, tg in enumerate(targets):
            idx = np.nonzero(st[k] == 1)[0]
            tg.set_keypoints(xy[k][idx])
            b, sb, _ = hip.lk_track(ctx, tg, [f1], fopt)
            if rep == 0:      # warm-up round: compare
                d = b[0] - kps[idx]
                keep = (sb[0] == 1) & ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) <= thr2)
                final = np.zeros(len(kps), np.uint8)
                final[idx] = keep
                agree = agree and np.array_equal(final, fst[k]) and np.array_equal(b[0], bxy[k][idx]) and np.array_equal(sb[0], bst[k][idx])
        if rep > 0:
            comp_ms += ctx.timing()["lk"][1]
    ctx.enable_timing(False)
    fwd_rows, kept_rows = int((st == 1).sum()), int((fst == 1).sum())
    return {"threshold": thr, "forward_ms": fwd_ms, "backward_ms": back_ms, "forward_plus_backward_ms": fwd_ms + back_ms,
            "backward_over_forward": back_ms / fwd_ms if fwd_ms else None, "composition_8_launches_ms": comp_ms / max(1, reps),
            "composition_note": "LK launches only: the eight set_keypoints uploads and spatial-bin launches the composition also needs are outside the timer",
            "composition_agrees_bitwise": bool(agree), "forward_rows": fwd_rows, "kept_rows": kept_rows,
            "dropped_fraction": (fwd_rows - kept_rows) / max(1, fwd_rows), "status_b_zero": int(((st == 1) & (bst == 0)).sum())}


def corr_timing(ctx, hip, f1, targets, fopt, thr, reps, xy, st, err):
    """forward + correlation launch of pc_lk_track_correlated; the check must leave the forward values alone"""
    cxy, cst, cerr, _ = hip.lk_track_correlated(ctx, f1, targets, thr, opt=fopt, corr=False)      # warm-up + the output that is compared
    assert np.array_equal(cxy, xy) and np.array_equal(cerr, err) and not (cst & ~st).any(), "the check changed a forward value"
    ctx.enable_timing(["lk", "lk_corr"])
    ctx.reset_timing()
    for _ in range(reps):
        hip.lk_track_correlated(ctx, f1, targets, thr, opt=fopt, corr=False)
    t = ctx.timing()
    ctx.enable_timing(False)
    fwd_ms, corr_ms = t["lk"][1] / max(1, t["lk"][0]), t["lk_corr"][1] / max(1, t["lk_corr"][0])
    fwd_rows, kept_rows = int((st == 1).sum()), int((cst == 1).sum())
    return {"threshold": thr, "forward_ms": fwd_ms, "correlation_ms": corr_ms, "correlation_over_forward": corr_ms / fwd_ms if fwd_ms else None,
            "forward_rows": fwd_rows, "kept_rows": kept_rows, "dropped_fraction": (fwd_rows - kept_rows) / max(1, fwd_rows)}


def norm_timing(ctx, hip, f1, targets, fopt, fb, reps, plain_ms, st):
    """forward (and, with fb > 0, backward) launch of pc_lk_track_normalized with the option on, against the plain launches of the
    same build: the forward one measured by the caller, the backward one measured here"""
    res = hip.lk_track_normalized(ctx, f1, targets, 1, 0.0, fb, -1, fopt)      # warm-up + the output that is compared
    off = hip.lk_track_normalized(ctx, f1, targets, 0, 0.0, fb, -1, fopt)
    hsh = hashlib.sha256()
    for a in res:
        hsh.update(np.ascontiguousarray(a).tobytes())
    out = {"rows": int((res[1] == 1).sum()), "rows_option_off": int((off[1] == 1).sum()), "sha256": hsh.hexdigest()[:16]}
    for name, flag in (("plain", 0), ("normalized", 1)):
        ctx.enable_timing(["lk", "lk_fb"])
        ctx.reset_timing()
        for _ in range(reps):
            again = hip.lk_track_normalized(ctx, f1, targets, flag, 0.0, fb, -1, fopt)
        t = ctx.timing()
        ctx.enable_timing(False)
        assert all(np.array_equal(a, b) for a, b in zip(again, res if flag else off)), "results vary between launches"
        out[name + "_forward_ms"] = t["lk"][1] / max(1, t["lk"][0])
        if fb > 0:
            out[name + "_backward_ms"] = t["lk_fb"][1] / max(1, t["lk_fb"][0])
    out["forward_over_plain"] = out["normalized_forward_ms"] / out["plain_forward_ms"] if out["plain_forward_ms"] else None
    out["forward_over_plain_of_the_first_loop"] = out["normalized_forward_ms"] / plain_ms if plain_ms else None
    if fb > 0:
        out["fb_threshold"] = fb
        out["backward_over_plain"] = out["normalized_backward_ms"] / out["plain_backward_ms"] if out["plain_backward_ms"] else None
    return out


def affine_timing(ctx, hip, f1, targets, fopt, reps, xy, st, err):
    """forward + refinement launch of pc_lk_track_affine against the forward launch alone (affine = 0) in alternating rounds; both
    launches are timed under class "lk", so the refinement's time is the difference of the class totals"""
    res = hip.lk_track_affine(ctx, f1, targets, 1, opt=fopt)      # warm-up + the output that is compared
    off = hip.lk_track_affine(ctx, f1, targets, 0, opt=fopt)
    assert np.array_equal(off[0], xy) and np.array_equal(off[1], st) and np.array_equal(off[2], err), "affine = 0 changed a forward value"
    assert np.array_equal(res[1], st), "the refinement changed a status"
    hsh = hashlib.sha256()
    for a in res:
        hsh.update(np.ascontiguousarray(a).tobytes())
    ms, launches = {0: 0.0, 1: 0.0}, {0: 0, 1: 0}
    ctx.enable_timing(["lk"])
    for _ in range(reps):
        for flag in (0, 1):
            ctx.reset_timing()
            again = hip.lk_track_affine(ctx, f1, targets, flag, opt=fopt)
            t = ctx.timing()["lk"]
            launches[flag] += t[0]
            ms[flag] += t[1]
    ctx.enable_timing(False)
    assert all(np.array_equal(a, b) for a, b in zip(again, res)), "results vary between launches"
    assert launches[0] == reps and launches[1] == 2 * reps, launches
    fwd_ms, aff_ms = ms[0] / reps, (ms[1] - ms[0]) / reps
    state = res[6]
    fwd_rows, accepted = int((st == 1).sum()), int((state == 1).sum())
    moved = np.hypot(*(res[0] - xy)[state == 1].T)
    return {"forward_ms": fwd_ms, "affine_ms": aff_ms, "affine_over_forward": aff_ms / fwd_ms if fwd_ms else None, "forward_rows": fwd_rows,
            "accepted_rows": accepted, "accepted_fraction": accepted / max(1, fwd_rows),
            "median_move_px": float(np.median(moved)) if accepted else None, "sha256": hsh.hexdigest()[:16]}


def search_timing(ctx, hip, f1, targets, fopt, reps, radius, xy, st, err):
    """forward + search launch of pc_lk_track_search against the forward launch alone (search_radius = 0) in alternating rounds; both
    launches are timed under class "lk", so the search's time is the difference of the class totals"""
    res = hip.lk_track_search(ctx, f1, targets, radius, opt=fopt)      # warm-up + the output that is compared
    off = hip.lk_track_search(ctx, f1, targets, 0, opt=fopt)
    assert np.array_equal(off[0], xy) and np.array_equal(off[1], st) and np.array_equal(off[2], err), "search_radius = 0 changed a forward value"
    hsh = hashlib.sha256()
    for a in res:
        hsh.update(np.ascontiguousarray(a).tobytes())
    ms, launches = {0: 0.0, 1: 0.0}, {0: 0, 1: 0}
    ctx.enable_timing(["lk"])
    for _ in range(reps):
        for flag in (0, 1):
            ctx.reset_timing()
            again = hip.lk_track_search(ctx, f1, targets, radius * flag, opt=fopt)
            t = ctx.timing()["lk"]
            launches[flag] += t[0]
            ms[flag] += t[1]
    ctx.enable_timing(False)
    assert all(np.array_equal(a, b) for a, b in zip(again, res)), "results vary between launches"
    assert launches[0] == reps and launches[1] == 2 * reps, launches
    fwd_ms, search_ms = ms[0] / reps, (ms[1] - ms[0]) / reps
    state = res[8]
    return {"search_radius": radius, "forward_ms": fwd_ms, "search_ms": search_ms, "search_over_forward": search_ms / fwd_ms if fwd_ms else None,
            "pairs": int(state.size), "state_0": int((state == 0).sum()), "state_1": int((state == 1).sum()), "state_2": int((state == 2).sum()),
            "forward_rows": int((st == 1).sum()), "rows_with_search": int((res[1] == 1).sum()), "sha256": hsh.hexdigest()[:16]}


def mask_polygon(w, h, fraction):
    """an ellipse-like 32-gon around the frame's centre that covers `fraction` of the frame (0 < fraction <= 0.75)"""
    s = np.sqrt(fraction / np.pi)
    a = 2.0 * np.pi * np.arange(32) / 32
    return np.stack([w / 2 + w * s * np.cos(a), h / 2 + h * s * np.sin(a)], axis=1).astype(np.float32)


def wmask_timing(ctx, hip, f1, targets, fopt, fb, reps, xy, st, err):
    """forward + masked launch of pc_lk_track_window_masked against the forward launch alone (mask_windows = 0) in alternating
    rounds; the backward launch of either variant has its own class"""
    res = hip.lk_track_window_masked(ctx, f1, targets, 1, fb, -1, fopt)      # warm-up + the output that is compared
    off = hip.lk_track_window_masked(ctx, f1, targets, 0, fb, -1, fopt)
    assert np.array_equal(off[0], xy) and np.array_equal(off[2], err), "mask_windows = 0 changed a forward value"
    touched = res[5] == 1
    assert np.array_equal(res[0][:, ~touched], xy[:, ~touched]) and np.array_equal(res[2][:, ~touched], err[:, ~touched]), "an untouched record changed"
    hsh = hashlib.sha256()
    for a in res:
        hsh.update(np.ascontiguousarray(a).tobytes())
    ms = {0: {"lk": 0.0, "lk_fb": 0.0}, 1: {"lk": 0.0, "lk_fb": 0.0}}
    launches = {0: 0, 1: 0}
    ctx.enable_timing(["lk", "lk_fb"])
    for _ in range(reps):
        for flag in (0, 1):
            ctx.reset_timing()
            again = hip.lk_track_window_masked(ctx, f1, targets, flag, fb, -1, fopt)
            t = ctx.timing()
            launches[flag] += t["lk"][0]
            for k in ms[flag]:
                ms[flag][k] += t[k][1]
    ctx.enable_timing(False)
    assert all(np.array_equal(a, b) for a, b in zip(again, res)), "results vary between launches"
    assert launches[0] == reps and launches[1] == 2 * reps, launches
    fwd_ms, masked_ms = ms[0]["lk"] / reps, (ms[1]["lk"] - ms[0]["lk"]) / reps
    out = {"forward_ms": fwd_ms, "masked_launch_ms": masked_ms, "forward_plus_masked_ms": fwd_ms + masked_ms,
           "masked_over_forward": masked_ms / fwd_ms if fwd_ms else None, "keypoints": int(len(touched)), "touched": int(touched.sum()),
           "touched_fraction": float(touched.mean()) if len(touched) else None, "forward_rows": int((st == 1).sum()),
           "rows_with_mask_windows": int((res[1] == 1).sum()), "rows_option_off": int((off[1] == 1).sum()), "sha256": hsh.hexdigest()[:16]}
    if fb > 0:
        out.update(fb_threshold=fb, plain_backward_ms=ms[0]["lk_fb"] / reps, weighted_backward_ms=ms[1]["lk_fb"] / reps)
        out["backward_over_plain"] = out["weighted_backward_ms"] / out["plain_backward_ms"] if out["plain_backward_ms"] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frame", type=int, default=100)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--arith", default="canonical", choices=["canonical", "lk_x86", "sobel_fma", "opencv_x86"])
    ap.add_argument("--max-iters", type=int, default=30, help="term_max_iters (30 = the reference's default); smaller values CUT the "
                    "stragglers' iterations off -- wrong results, but the time saved is the ceiling of what deferring them could gain")
    ap.add_argument("--fb", type=float, default=0.0, metavar="PX", help="also time the forward-backward check at this threshold")
    ap.add_argument("--min-correlation", type=float, default=0.0, metavar="V", help="also time the minimum-correlation check at this threshold")
    ap.add_argument("--normalize", action="store_true", help="also time the brightness-normalised launch (with --fb: and its backward launch)")
    ap.add_argument("--affine", action="store_true", help="also time the affine refinement launch beside the forward launch")
    ap.add_argument("--search-radius", type=int, default=0, metavar="N", help="also time the search prepass launch at this radius beside the forward launch")
    ap.add_argument("--mask-fraction", type=float, default=0.0, metavar="F",
                    help="polygon mask over this fraction of the frame (0 < F <= 0.75) on frame1, before its detection, and on the targets")
    ap.add_argument("--mask-windows", action="store_true", help="also time the masked windows beside the forward launch (needs --mask-fraction)")
    ap.add_argument("--shift", type=int, nargs=2, default=None, metavar=("DX", "DY"),
                    help="targets = frame1 rolled by whole pixels, (k DX / 8, k DY / 8) for skip k, instead of the clip's frames")
    args = ap.parse_args()
    if args.mask_windows and not args.mask_fraction > 0:
        ap.error("--mask-windows needs --mask-fraction")
    if args.mask_fraction and not 0 < args.mask_fraction <= 0.75:
        ap.error("--mask-fraction must be in (0, 0.75]")

    import torch
    from polychase_amd import hip, synth

    w, h, max_level = CONFIGS[args.config]
    dev = torch.device("cuda", 0)
    clip = synth.NoiseClip(w, h, 300, device=str(dev))
    ctx = hip.Context(0)
    ctx.set_arithmetic({"canonical": hip.ARITH_CANONICAL, "lk_x86": hip.ARITH_LK_X86_ORDER, "sobel_fma": hip.ARITH_SOBEL_FMA,
                        "opencv_x86": hip.ARITH_OPENCV_X86}[args.arith])
    fopt = hip.flow_options(max_level=max_level, window_size=args.window, term_max_iters=args.max_iters)
    frames = {}
    for s in (0,) + SKIPS:
        f = hip.Frame(ctx, w, h, args.window, max_level)
        img = clip.frame_torch(args.frame + (0 if args.shift else s))
        if args.shift and s:
            img = torch.roll(img, (s * args.shift[1] // 8, s * args.shift[0] // 8), (0, 1))
        f.set_rgb(img)
        if args.mask_fraction > 0:
            f.set_mask_polygons([mask_polygon(w, h, args.mask_fraction)])
        frames[s] = f
    f1 = frames[0]
    f1.detect()
    n = f1.num_keypoints
    targets = [frames[s] for s in SKIPS]
    xy, st, err = hip.lk_track(ctx, f1, targets, fopt)          # warm-up + reference output
    for _ in range(3):
        hip.lk_track(ctx, f1, targets, fopt)
    ctx.enable_timing(["lk"])
    ctx.reset_timing()
    for _ in range(args.reps):
        xy2, st2, err2 = hip.lk_track(ctx, f1, targets, fopt)
    launches, ms = ctx.timing()["lk"]
    ctx.enable_timing(False)
    ctx.lk_profile()   # discard: the timed launches below are profiled on their own
    hip.lk_track(ctx, f1, targets, fopt)
    assert np.array_equal(xy, xy2) and np.array_equal(st, st2) and np.array_equal(err, err2), "results vary between launches"
    filt = hip.lk_track_filtered(ctx, f1, targets, fopt)
    hsh = hashlib.sha256()
    for a in (xy, st, err):
        hsh.update(np.ascontiguousarray(a).tobytes())
    for idx, fxy, ferr in filt:
        for a in (idx, fxy, ferr):
            hsh.update(np.ascontiguousarray(a).tobytes())
    # the filtered path must be the status==1 rows of the raw one
    for t, (idx, fxy, ferr) in enumerate(filt):
        keep = np.nonzero(st[t] == 1)[0]
        assert np.array_equal(idx, keep.astype(np.uint32)) and np.array_equal(fxy, xy[t][keep]) and np.array_equal(ferr, err[t][keep])
    x86_stats = None
    if ctx.arithmetic & hip.ARITH_LK_X86_ORDER:   # one more launch with the diagnostics counters on
        ctx.lk_x86_stats(True)
        hip.lk_track(ctx, f1, targets, fopt)
        x86_stats = ctx.lk_x86_stats(False)
    out = {"config": args.config, "window": args.window, "arith": args.arith, "max_iters": args.max_iters, "keypoints": n, "launches": launches,
           "lk_ms_per_launch": ms / max(1, launches), "tracked_rows": int((st == 1).sum()),
           "sha256": hsh.hexdigest()[:16], "lib": os.environ.get("POLYCHASE_HIP_LIB", "default")}
    if x86_stats is not None:
        out["x86_stats_one_launch"] = x86_stats
    if args.normalize:
        out["normalize"] = norm_timing(ctx, hip, f1, targets, fopt, args.fb, args.reps, ms / max(1, launches), st)
    if args.affine:
        out["affine"] = affine_timing(ctx, hip, f1, targets, fopt, args.reps, xy, st, err)
    if args.mask_fraction > 0:
        out["mask_fraction"] = args.mask_fraction
    if args.mask_windows:
        out["mask_windows"] = wmask_timing(ctx, hip, f1, targets, fopt, args.fb, args.reps, xy, st, err)
    if args.search_radius > 0:
        out["search"] = search_timing(ctx, hip, f1, targets, fopt, args.reps, args.search_radius, xy, st, err)
    if args.min_correlation > 0:      # (before --fb: that one leaves other keypoints on the target frames)
        out["min_correlation"] = corr_timing(ctx, hip, f1, targets, fopt, args.min_correlation, args.reps, xy, st, err)
    if args.fb > 0:
        out["fb"] = fb_timing(ctx, hip, f1, targets, fopt, args.fb, args.reps, xy, st, err)
    prof = ctx.lk_profile()
    if any(prof):
        names = ["i_stage", "i_eval", "pickup", "j_stage", "iterate", "err", "life", "waves", "wave_iters", "stagings"]
        w = max(1, prof[7])
        out["profile_cycles_per_wave"] = {n: round(v / w, 1) for n, v in zip(names, prof)}
    print(json.dumps(out), flush=True)
    for f in frames.values():
        f.close()
    ctx.close()


if __name__ == "__main__":
    main()
