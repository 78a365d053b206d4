#!/usr/bin/env python3
"""prep_chain.py -- the frame-preparation chain in a `rocprofv3 --kernel-trace` CSV of bench.py: per frame, the
kernels of the preparation queue from the first level<0> launch to the LK visiting order (bin_scatter), their
durations beside LK, the gaps between them, and how the LK launches line up behind the chain.

    python tools/prep_chain.py <kernel_trace.csv> [--json]

Frames: the queue that runs level_kernel<0> is the preparation queue; a frame's chain starts at the first level<0>
after the previous frame's last chain kernel and ends at bin_scatter_kernel.  The first quarter of the frames is
skipped (warm-up).  "lk_after_chain_us": for every LK launch, its start minus the end of the newest chain that ended
before it -- an LK launch that waits for its frame's keypoints starts a few microseconds after that end.
"""
import csv
import json
import statistics as st
import sys

LAST = "bin_scatter_kernel"


def short(name):
    n = name.split("(")[0]
    return n.replace("void ", "").replace("pc::", "")


def main():
    path = sys.argv[1]
    rows = list(csv.DictReader(open(path)))
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], short(r["Kernel_Name"])) for r in rows)
    prep_q = next(q for s, e, q, n in ev if n.startswith("level_kernel<0>"))
    prep = [x for x in ev if x[2] == prep_q and not x[3].startswith("__amd")]
    lk = [x for x in ev if x[3].startswith("lk3_kernel") or x[3].startswith("lk4")]
    frames, cur = [], []
    for x in prep:
        cur.append(x)
        if x[3] == LAST:
            if any(y[3].startswith("min_eig") for y in cur):
                frames.append(cur)
            cur = []
    frames = frames[len(frames) // 4:]
    chain = [(f[-1][1] - f[0][0]) / 1e3 for f in frames]
    post = []   # from the end of min_eig (response map + cell maxima) to the end of bin_scatter
    per = {}
    gaps = {}
    for f in frames:
        me = next(i for i, y in enumerate(f) if y[3].startswith("min_eig"))
        post.append((f[-1][1] - f[me][1]) / 1e3)
        for a, b in zip(f, f[1:]):
            gaps.setdefault(b[3], []).append((b[0] - a[1]) / 1e3)
        for y in f:
            per.setdefault(y[3], []).append((y[1] - y[0]) / 1e3)
    ends = [f[-1][1] for f in frames]
    t_lo, t_hi = frames[0][0][0], frames[-1][-1][1]
    waits = []
    j = 0
    for s, e, q, n in lk:
        if s < t_lo or s > t_hi:
            continue
        while j + 1 < len(ends) and ends[j + 1] <= s:
            j += 1
        if ends[j] <= s:
            waits.append((s - ends[j]) / 1e3)
    period = (frames[-1][-1][1] - frames[0][-1][1]) / 1e3 / max(1, len(frames) - 1)
    out = {
        "frames": len(frames),
        "frame_period_us": round(period, 1),
        "chain_us_median": round(st.median(chain), 1),
        "chain_us_p90": round(sorted(chain)[int(0.9 * (len(chain) - 1))], 1),
        "after_min_eig_us_median": round(st.median(post), 1),
        "kernels_per_frame": round(sum(len(f) for f in frames) / len(frames), 2),
        "kernel_us_median": {k: round(st.median(v), 1) for k, v in per.items()},
        "gap_before_us_median": {k: round(st.median(v), 1) for k, v in gaps.items()},
        "lk_launches": len(waits),
        "lk_after_chain_us_median": round(st.median(waits), 1) if waits else None,
        "lk_within_15us_of_chain_end": round(sum(w < 15.0 for w in waits) / max(1, len(waits)), 3),
    }
    if "--json" in sys.argv:
        print(json.dumps(out))
        return
    for k, v in out.items():
        print(f"{k}: {v}")


if __name__ == "__main__":
    main()
