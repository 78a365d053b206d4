"""CPU: every scene of tests/gftt_dot_scenes.py meets the condition it is named for, on the oracle alone -- the candidate
count, the bucket histogram with its group sums and shift, the squared distances, the number of higher-priority neighbours
within the radius, which candidates share a 64-candidate step -- and the oracle and tests/masked_gftt_ref.py agree on every
scene.  A scene that no longer meets its condition fails HERE, not silently on the GPU (tests/test_gftt_edges_gpu.py).

Then what the scenes are for: three mutated copies of the numpy restatement of the detector (made in this file; the product
is not touched) -- `<=` in the radius predicate, ties ordered by ascending address, truncation to max_corners + 1 -- and how
many keypoints of every scene change under each, beside the 320 x 240 noise frame of test_gpu_parity.py::test_gftt_options.
The table is profiles/gftt_edge_scenes.txt; running this file as a script rewrites it, the test holds it to the code."""
import os
import sys

import numpy as np
import pytest

import gftt_dot_scenes as S
import masked_gftt_ref as ref
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "gftt_edge_scenes.txt")


def _hist(name, run):
    return S.histogram(S.scene(name), run)


def _dots_are_the_candidates(name, run):
    sc = S.scene(name)
    _, xs, ys = S.ordered_candidates(sc, run)
    assert S.expected(name, run)[2] == len(sc.dots) == len(xs)
    assert set(zip(xs.tolist(), ys.tolist())) == {(x, y) for x, y, _ in sc.dots}


def _order_index(sc, run):
    """(x, y) -> position in processing order"""
    _, xs, ys = S.ordered_candidates(sc, run)
    return {(int(x), int(y)): k for k, (x, y) in enumerate(zip(xs, ys))}


# ---- every scene: the oracle and the numpy restatement agree --------------------------------------------------------------
@pytest.mark.parametrize("name,run", S.cases(), ids=lambda v: str(v))
def test_oracle_and_numpy_reference_agree(name, run):
    sc = S.scene(name)
    opt = S.options(sc, run)
    xy, _, ncand = oracle.gftt(sc.gray, opt, want_eig=True)
    rxy, eig, rncand = ref.gftt(sc.gray, opt, None if sc.mask is None else np.full(sc.gray.shape, 7, np.uint8))
    assert ncand == rncand
    assert np.array_equal(xy, rxy), "keypoints in value and order"
    vals, xs, ys = S.ordered_candidates(sc, run)
    if sc.mask is None:
        cv, ci = ref.candidates(eig, opt, None)
        assert np.array_equal(ci, ys * sc.w + xs) and np.array_equal(cv, vals)
    assert np.all(np.diff(vals.astype(np.float64)) <= 0), "processing order: value descending"


# ---- the sort's edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(S.scene("group_over_lds").runs))
def test_group_over_lds(run):
    _dots_are_the_candidates("group_over_lds", run)
    b, hist, groups, shift = _hist("group_over_lds", run)
    assert hist.max() <= S.BUCKET_SLOTS, "no bucket anywhere above 512"
    big = np.nonzero(groups > S.BUCKET_SLOTS)[0]
    assert len(big) >= 1, "one aligned group of four buckets holds more than 512 keys"
    for g in big:
        assert np.count_nonzero(hist[4 * g:4 * g + 4]) >= 2, "at least two non-empty buckets in the group"
    if run == "q1e-8":
        assert shift == 15 and np.nonzero(hist)[0].tolist() == [0, 2, 5, 7] and hist[[0, 2, 5, 7]].tolist() == [300] * 4
        assert groups[0] == 600 and groups[1] == 600


@pytest.mark.parametrize("name,full", [("bucket_512", 512), ("bucket_513", 513), ("bucket_513_masked", 512)])
def test_bucket_512_513(name, full):
    sc = S.scene(name)
    run = "q1e-20"
    b, hist, groups, shift = _hist(name, run)
    assert hist.max() == full and hist[0] == full and S.expected(name, run)[2] == full + 400
    assert np.count_nonzero(hist[0:4]) == 2 and hist[3] == 400, "a second non-empty bucket in the same group of four"
    assert groups[0] == full + 400 > S.BUCKET_SLOTS, "the group takes the bucket-by-bucket branch"
    assert np.count_nonzero(hist) == 2
    if sc.mask is None:
        _dots_are_the_candidates(name, run)
        return
    # the mask removes exactly one dot, one of the full bucket; without it the bucket overflows
    assert np.count_nonzero(sc.mask == 0) == 1
    mx, my = sc.marks["masked_dot"]
    assert sc.gray[my, mx] == 255 and sc.mask[my, mx] == 0
    assert oracle.gftt(sc.gray, S.options(sc, run), want_eig=True)[2] == 913
    xy = S.expected(name, run)[0]
    assert len(xy) == 912 and not np.any((xy[:, 0] == mx) & (xy[:, 1] == my))
    assert np.array_equal(S.scene("bucket_513").gray, sc.gray)


# ---- counts on the workgroup edge -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_counts(n):
    name = "count_%d" % n
    sc = S.scene(name)
    assert {"table5", "accept_all", "large70"} <= set(sc.runs)
    for run in ("table5", "accept_all", "large70") + (("table5_harris",) if n == 257 else ()):
        _dots_are_the_candidates(name, run)
        b, hist, groups, shift = _hist(name, run)
        assert groups.max() <= 64, "no bucket or group comes near 512"
    assert (n - 1) // S.SUP_BLOCK == (0 if n <= 256 else 1)
    assert len(S.expected(name, "table5")[0]) == n == len(S.expected(name, "accept_all")[0])
    assert 1 <= len(S.expected(name, "large70")[0]) <= 4
    assert not 0.5 >= 1 and 5.0 <= S.TABLE_MAX_RADIUS < 70.0      # accept_all_kernel, the table kernel, the grid kernel
    if n == 257:
        assert len(S.expected(name, "max1")[0]) == 1 == len(S.expected(name, "max1_large70")[0])
    if n == 256:
        assert S.expected(name, "quality1")[2] == 0 and len(S.expected(name, "quality1")[0]) == 0


# ---- the radius predicate on its boundary ---------------------------------------------------------------------------------
def _d2(p, q):
    return (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2


def test_radius_table_pairs():
    name = "radius_table_3_4_5"
    sc = S.scene(name)
    pairs = sc.marks["pairs"]
    _dots_are_the_candidates(name, "r5")
    pos = [(x, y) for x, y, _ in sc.dots]
    for p, q, r in pairs:
        assert _d2(p, q) == r * r
        assert float(np.float32(_d2(p, q))) == float(r) * float(r) < S.up(r) * S.up(r), "kept at r, in conflict at the next double"
        for o in pos:
            assert o in (p, q) or (_d2(o, p) > 14 * 14 and _d2(o, q) > 14 * 14), "nothing but the partner within the largest radius"
    for a, b, r in S.TRIPLES:
        n_r = sum(1 for p in pairs if p[2] == r)
        closer = sum(1 for p in pairs if p[2] < r)
        assert n_r == 6
        at, above = S.expected(name, "r%d" % r)[0], S.expected(name, "r%d_up" % r)[0]
        assert len(at) == len(pos) - closer and len(above) == len(at) - n_r
        assert float(r) <= S.TABLE_MAX_RADIUS and S.up(r) <= S.TABLE_MAX_RADIUS
    # the member that goes is the one of lower priority: lower value, or the lower address of equals
    above = {tuple(p) for p in S.expected(name, "r13_up")[0].astype(int).tolist()}
    val = {(x, y): b for x, y, b in sc.dots}
    for p, q, r in pairs:
        first = max((p, q), key=lambda t: (val[t], t[1] * sc.w + t[0]))
        assert first in above and (p if first == q else q) not in above
    assert any(val[p] == val[q] for p, q, _ in pairs) and any(val[p] != val[q] for p, q, _ in pairs)


@pytest.mark.parametrize("name,r", [("radius_64", 64), ("radius_65", 65)])
def test_radius_lattices(name, r):
    sc = S.scene(name)
    at, above = "r%d" % r, "r%d_up" % r
    _dots_are_the_candidates(name, at)
    n = len(sc.dots)
    assert n > S.SUP_BLOCK, "more than one suppression workgroup"
    pos = np.array([(x, y) for x, y, _ in sc.dots], np.int64)
    d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, 1 << 40)
    assert d2.min() == r * r and np.all(d2.min(1) == r * r), "every dot has a neighbour at distance exactly r, none closer"
    assert len(S.expected(name, at)[0]) == n and len(S.expected(name, above)[0]) < n // 2
    assert (float(r) > S.TABLE_MAX_RADIUS) == (r == 65) and S.up(r) > S.TABLE_MAX_RADIUS
    for run in (at, above):
        assert _hist(name, run)[2].max() <= 64


def test_radius_65_pairs_straddle_cells_and_steps():
    name = "radius_65"
    sc = S.scene(name)
    pairs = sc.marks["pairs"]
    assert sorted((abs(q[0] - p[0]), abs(q[1] - p[1])) for p, q, _ in pairs) == sorted(S.PAIR_OFFSETS_65)
    order = _order_index(sc, "r65")
    pos = [(x, y) for x, y, _ in sc.dots]
    kept = {tuple(p) for p in S.expected(name, "r65_up")[0].astype(int).tolist()}
    steps = []
    for p, q, r in pairs:
        assert _d2(p, q) == 65 * 65
        assert p[0] // 65 != q[0] // 65 and p[1] // 65 != q[1] // 65, "the members lie in different grid cells, in x and in y"
        assert all(o in (p, q) or (_d2(o, p) > 66 * 66 and _d2(o, q) > 66 * 66) for o in pos)
        steps.append((order[p] // S.LARGE_STEP, order[q] // S.LARGE_STEP))
        first, second = (p, q) if order[p] < order[q] else (q, p)
        assert first in kept and second not in kept
    assert steps[:3] == [(0, 0)] * 3, "both members in one 64-candidate step"
    assert steps[3] == (0, 1) and order[pairs[3][0]] == 63 and order[pairs[3][1]] == 64, "... and in two consecutive steps"
    assert len(S.expected(name, "r65")[0]) == len(pos)


# ---- ties -------------------------------------------------------------------------------------------------------------------
def _higher_priority_neighbours(sc, run):
    opt = S.options(sc, run)
    _, xs, ys = S.ordered_candidates(sc, run)
    pos = np.stack([xs, ys], 1).astype(np.float32)
    d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(2).astype(np.float32)
    near = d2.astype(np.float64) < opt.min_distance * opt.min_distance
    return np.array([np.count_nonzero(near[k, :k]) for k in range(len(pos))])


@pytest.mark.parametrize("w", [156, 155])
def test_ties(w):
    name = "ties_500_w%d" % w
    sc = S.scene(name)
    assert w % 4 == (0 if w == 156 else 3)
    for run in sc.runs:
        _dots_are_the_candidates(name, run)
        vals, xs, ys = S.ordered_candidates(sc, run)
        assert len(vals) == 500 and len(np.unique(vals)) == 1
        assert np.all(np.diff(ys * w + xs) < 0), "equal responses: descending address"
        kp = S.expected(name, run)[0]
        assert np.all(np.diff(kp[:, 1].astype(np.int64) * w + kp[:, 0].astype(np.int64)) < 0), "keypoints come out in that order too"
        assert _hist(name, run)[1].max() == 500 <= S.BUCKET_SLOTS
    counts = [len(S.expected(name, run)[0]) for run in ("r6", "r6_up", "r13", "r19", "r6_up_harris")]
    assert counts[0] == 500 and counts[1] == 250 == counts[4] and counts[3] < counts[2] < 250
    # the 12-neighbour cache: at 13.0 a lane has at most 6 higher-priority neighbours at this pitch (12 dots within the radius:
    # it fits), at 19.0 most have 18 (36 within the radius)
    assert _higher_priority_neighbours(sc, "r6").max() == 0
    assert _higher_priority_neighbours(sc, "r13").max() == 6
    n19 = _higher_priority_neighbours(sc, "r19")
    assert n19.max() == 18 > S.SUP_NB and np.count_nonzero(n19 > S.SUP_NB) >= 350


# ---- the frame's border -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", S.BORDER_SIZES)
def test_border_ring(w, h):
    name = "border_ring_%dx%d" % (w, h)
    sc = S.scene(name)
    xs, ys = {x for x, _, _ in sc.dots}, {y for _, y, _ in sc.dots}
    assert {0, 1, w - 2, w - 1} <= xs and {0, 1, h - 2, h - 1} <= ys
    assert sc.runs["grid5x3"] == dict(grid_rows=3, grid_cols=5)
    for run in sc.runs:
        _, cx, cy = S.ordered_candidates(sc, run)
        assert len(cx) > 0 and np.all((cx >= 1) & (cx <= w - 2) & (cy >= 1) & (cy <= h - 2)), "strictly interior"
        assert cx.min() <= 2 and cx.max() >= w - 3 and cy.min() <= 2 and cy.max() >= h - 3, "candidates next to all four borders"
        assert np.any((cx == 1) | (cx == w - 2) | (cy == 1) | (cy == h - 2)), "the first interior ring is used"
        assert S.expected(name, run)[2] == len(cx)


# ---- the keypoint buffer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_keypoint_counts(n):
    name = "keypoints_%d" % n
    for run, limit in (("max0", 0), ("max4096", 4096), ("max5000", 5000)):
        _dots_are_the_candidates(name, run)
        assert S.scene(name).runs[run]["min_distance"] == 0.0 and S.scene(name).runs[run]["max_corners"] == limit
        assert len(S.expected(name, run)[0]) == (min(n, limit) if limit else n)
        assert _hist(name, run)[2].max() <= 256


@pytest.mark.parametrize("n", [7167, 7168, 7169])
def test_keypoint_capacity_counts(n):
    """the real edge of the keypoint buffer: 256 x 256 is the largest frame with the smallest buffer"""
    name = "keypoint_capacity_%d" % n
    sc = S.scene(name)
    assert sc.w * sc.h // 16 == 4096 and 4096 + 4096 // 2 + 1024 == S.CAPACITY
    for run, limit in (("max0", 0), ("max8000", 8000), ("max7168", S.CAPACITY), ("max5000", 5000)):
        xy, _, ncand = S.expected(name, run)
        assert ncand == n and len(xy) == (min(n, limit) if limit else n)
        assert _hist(name, run)[1].max() <= S.BUCKET_SLOTS and _hist(name, run)[2].max() <= S.BUCKET_SLOTS


# ---- the analyzer's clips ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_edge", [4096, 4097])
def test_hint_clips(n_edge):
    frames = S.hint_clip(n_edge)
    assert len(frames) == S.HINT_LEAD + S.HINT_EDGE_FRAMES and S.HINT_LEAD >= 8 + 1 + 2, "the hint has settled before the edge frames are queued"
    for run, kw in S.HINT_RUNS.items():
        opt = oracle.gftt_options(**kw)
        for t, g in enumerate(frames):
            n, hist = S.frame_histogram(g, opt)
            assert n == (64 if t < S.HINT_LEAD else n_edge) and hist.max() <= 256
            assert n + n // 4 <= 4096 or t >= S.HINT_LEAD, "the lead frames leave the hint at its floor"
    assert not np.array_equal(frames[-1], frames[-2]), "the dots move from frame to frame"
    assert {"default", "accept_all", "large70"} == set(S.HINT_RUNS) and S.HINT_RUNS["default"] == {}


def test_bucket_and_ties_clips():
    for kw in (S.BUCKET_CLIP_GFTT, dict(min_distance=7.0, **S.BUCKET_CLIP_GFTT)):
        opt = oracle.gftt_options(**kw)
        for first in (512, 513):
            for t, g in enumerate(S.bucket_clip(first)):
                n, hist = S.frame_histogram(g, opt)
                assert hist.max() == (513 if (t + (first == 513)) % 2 else 512) and n == hist.max() + 400
    r7, r3 = oracle.gftt_options(min_distance=7.0, **S.BUCKET_CLIP_GFTT), oracle.gftt_options(min_distance=3.0, **S.BUCKET_CLIP_GFTT)
    assert all(len(oracle.gftt(g, r7)) < len(oracle.gftt(g, r3)) for g in S.bucket_clip()), "a redo with the wrong table shows"
    r7, r3 = oracle.gftt_options(min_distance=7.0, **S.ONE_CELL), oracle.gftt_options(min_distance=3.0, **S.ONE_CELL)
    for g in S.ties_clip():
        assert len(oracle.gftt(g, r7)) == 250 and len(oracle.gftt(g, r3)) == 500


# ---- what the scenes are for: mutations of the numpy restatement ---------------------------------------------------------------
def _mutant_gftt(gray, opt, mask, mutation):
    """masked_gftt_ref.gftt with one deliberate error"""
    h, w = gray.shape
    eig = ref.response(gray, opt)
    vals, idx = ref.candidates(eig, opt, mask)
    if mutation == "ties_ascending":
        order = np.lexsort((idx, -vals.astype(np.float64)))
        vals, idx = vals[order], idx[order]
    if mutation == "max_corners_plus_1" and opt.max_corners > 0:
        opt = oracle.gftt_options(**{k: getattr(opt, k) for k, _ in opt._fields_})
        opt.max_corners += 1
    if mutation == "radius_le" and opt.min_distance >= 1:
        return _suppress_le(idx, w, h, opt)
    return ref.suppress(idx, w, h, opt)


def _suppress_le(idx, w, h, opt):
    """masked_gftt_ref.suppress with `<=` where the reference has `<` (all pairs: the scenes are small)"""
    ys, xs = (idx // w).astype(np.float32), (idx % w).astype(np.float32)
    r2 = float(opt.min_distance) * float(opt.min_distance)
    kept = []
    for k in range(len(idx)):
        if kept:
            a = np.array(kept)
            dx, dy = xs[k] - xs[a], ys[k] - ys[a]
            if np.any((dx * dx + dy * dy).astype(np.float64) <= r2):
                continue
        kept.append(k)
        if opt.max_corners > 0 and len(kept) == opt.max_corners:
            break
    return np.stack([xs[kept], ys[kept]], 1).astype(np.float32).reshape(-1, 2)


MUTATIONS = ("radius_le", "ties_ascending", "max_corners_plus_1")


def _changed(a, b):
    """keypoints that differ, position by position, plus the difference in length"""
    n = min(len(a), len(b))
    return int(np.count_nonzero(np.any(a[:n] != b[:n], axis=1))) + abs(len(a) - len(b))


def _noise_rows():
    from polychase_amd import synth
    rgb = synth.NoiseClip(320, 240, 30).frame(3)
    gray = oracle.rgb2gray(rgb)
    rows = []
    for kw in [dict(), dict(max_corners=50), dict(min_distance=0.0), dict(min_distance=9.5, quality_level=0.05),
               dict(grid_rows=1, grid_cols=1), dict(grid_rows=7, grid_cols=9)]:
        opt = oracle.gftt_options(**kw)
        base = oracle.gftt(gray, opt)
        label = "noise_320x240 " + (",".join("%s=%s" % kv for kv in kw.items()) or "default")
        rows.append((label, len(base), [_changed(base, _mutant_gftt(gray, opt, None, m)) for m in MUTATIONS]))
    return rows


def _scene_rows():
    rows = []
    for name, run in S.cases():
        sc = S.scene(name)
        opt = S.options(sc, run)
        base = S.expected(name, run)[0]
        rows.append(("%s %s" % (name, run), len(base), [_changed(base, _mutant_gftt(sc.gray, opt, sc.mask, m)) for m in MUTATIONS]))
    return rows


def table_text():
    lines = ["# keypoints that change under a mutated copy of the numpy detector (tests/test_gftt_edges_cpu.py), per scene and run",
             "# columns: keypoints of the oracle | changed with `<=` in the radius predicate | with ties in ascending address order |",
             "#          with truncation to max_corners + 1",
             "%-52s %9s %10s %15s %19s" % ("scene run", "keypoints", "radius_le", "ties_ascending", "max_corners_plus_1")]
    for label, n, ch in _noise_rows() + _scene_rows():
        lines.append("%-52s %9d %10d %15d %19d" % (label, n, *ch))
    return "\n".join(lines) + "\n"


def test_mutation_table():
    scene_rows, noise_rows = _scene_rows(), _noise_rows()
    for k, m in enumerate(MUTATIONS):
        assert any(ch[k] > 0 for _, _, ch in scene_rows), "no scene notices " + m
    # the noise frame never sees a tie (it does meet distance 5 = 3-4-5 at the default radius, and not at 9.5)
    assert all(ch[1] == 0 for _, _, ch in noise_rows)
    # the scenes built for an edge notice its mutation
    by = {label: ch for label, _, ch in scene_rows}
    for label in ("radius_table_3_4_5 r5", "radius_table_3_4_5 r10", "radius_table_3_4_5 r13", "radius_64 r64", "radius_65 r65",
                  "ties_500_w156 r6", "ties_500_w155 r6"):
        assert by[label][0] > 0, label
    for label in ("ties_500_w156 r6_up", "ties_500_w155 r13", "ties_500_w156 r19"):
        assert by[label][1] > 0, label
    assert by["count_257 max1"][2] > 0 and by["keypoints_4097 max4096"][2] > 0
    assert os.path.exists(TABLE), "run tests/test_gftt_edges_cpu.py as a script to write profiles/gftt_edge_scenes.txt"
    assert open(TABLE).read() == table_text(), "profiles/gftt_edge_scenes.txt is out of date: run this file as a script"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    with open(TABLE, "w") as f:
        f.write(table_text())
    print(open(TABLE).read())
