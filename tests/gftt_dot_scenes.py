"""Dot scenes for the GFTT detection chain's structural edges.  TEST INFRASTRUCTURE ONLY.

A single bright pixel on black yields exactly one candidate (at the pixel) whose response depends only on its brightness,
as long as the dots keep a pitch of 5 px or more.  So the number of candidates, the value bucket each one falls into, the
distances between them and their order are all chosen here, by construction, and the chain's edges -- a value bucket of
exactly 512 keys, four buckets that only fit the sort's LDS buffer one at a time, two candidates at distance exactly
min_distance, a frame of equal responses, 255 / 256 / 257 candidates, a full keypoint buffer -- are met on purpose, not by
chance.

  scene(name), cases()   a Scene (built on first use): the image, an optional detection mask, and the option sets ("runs")
                         it is detected with; every (scene, run)
  hint_clip, bucket_clip, ties_clip   short clips of such frames for the analyzer
  expected(scene, run)   keypoints, response map and candidate count of the CPU oracle (of masked_gftt_ref with a mask)
  ordered_candidates     the candidates in processing order, from the oracle (tests/masked_gftt_ref.py: candidates)
  sort_range, buckets    a restatement, in integers, of the sort's bucket rule (kernels_gftt.hip: nms_kernel's value range,
                         make_sort_range, bucket_of), so that a scene can state which bucket every candidate falls into

tests/test_gftt_edges_cpu.py asserts on the oracle alone that every scene meets the condition it is named for.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import masked_gftt_ref as ref
import oracle

# the sort's constants (kernels.hpp, kernels_gftt.hip)
SORT_BUCKETS = 8192        # kSortBuckets
BUCKETS_PER_WAVE = 4       # kBucketsPerWave: an aligned group of four buckets is sorted by one wavefront
BUCKET_SLOTS = 512         # kBucketSlots == kBucketLds
SUP_BLOCK = 256            # candidates per suppression workgroup
SUP_NB = 12                # higher-priority neighbours a suppression lane caches
LARGE_STEP = 64            # candidates per step of suppress_large_radius_kernel
TABLE_MAX_RADIUS = 64.0    # kSuppressMaxTableRadius: above it the grid kernel


# ---- images ---------------------------------------------------------------------------------------------------------
def lattice(x0, y0, pitch, nx, ny, n=None):
    """the first n positions (row by row) of an nx x ny lattice"""
    pts = [(x0 + pitch * i, y0 + pitch * j) for j in range(ny) for i in range(nx)]
    return pts if n is None else pts[:n]


def dot_image(w, h, dots):
    """gray uint8 (h, w), black, with pixel (x, y) set to b for every (x, y, b) of dots"""
    g = np.zeros((h, w), np.uint8)
    for x, y, b in dots:
        assert 0 <= x < w and 0 <= y < h and g[y, x] == 0, (x, y, w, h)
        g[y, x] = b
    g.setflags(write=False)
    return g


def with_brightness(pts, classes):
    """dot k takes classes[k % len(classes)]: neighbours on the lattice differ, every class is spread over the frame"""
    return [(x, y, classes[k % len(classes)]) for k, (x, y) in enumerate(pts)]


@dataclass
class Scene:
    name: str
    gray: np.ndarray
    dots: list                                   # (x, y, brightness)
    runs: dict = field(default_factory=dict)     # run name -> keyword arguments of gftt_options
    mask: np.ndarray | None = None
    marks: dict = field(default_factory=dict)    # named positions the CPU conditions refer to

    @property
    def w(self):
        return self.gray.shape[1]

    @property
    def h(self):
        return self.gray.shape[0]


def up(x: float) -> float:
    """the next double above x"""
    return float(np.nextafter(np.float64(x), np.inf))


ONE_CELL = dict(grid_rows=1, grid_cols=1)


# ---- the scenes -----------------------------------------------------------------------------------------------------
def _group_over_lds():
    # 300 dots each of four neighbouring brightness values under a tiny quality level: the whole value range is 8192 buckets
    # of 2^15 ordered units, the four values land in one aligned group of four buckets, 1200 keys in all, 300 per bucket at most
    pts = lattice(3, 3, 5, 40, 30)
    dots = with_brightness(pts, (255, 254, 253, 252))
    # (Harris: the response goes with the fourth power of the brightness; 1e-12 brings two of the values into one group)
    return Scene("group_over_lds", dot_image(205, 156, dots), dots,
                 {"q1e-8": dict(quality_level=1e-8, **ONE_CELL), "harris_q1e-12": dict(quality_level=1e-12, use_harris=1, **ONE_CELL)})


def _bucket_edge(name, n_top, masked=False):
    # n_top dots of 255 (one bucket) and 400 of 250 (another bucket of the same group of four) at quality level 1e-20
    pts = lattice(3, 3, 5, 38, 25)
    n_all = n_top + 400
    order = np.random.default_rng(11).permutation(n_all)        # the two classes mixed over the frame
    cls = np.where(order < n_top, 255, 250)
    dots = [(x, y, int(b)) for (x, y), b in zip(pts[:n_all], cls)]
    gray = dot_image(195, 131, dots)
    sc = Scene(name, gray, dots, {"q1e-20": dict(quality_level=1e-20, **ONE_CELL)})
    if masked:
        # one dot of the full bucket masked out (not the first of its class in address order, not on the frame's edge)
        tops = [d for d in dots if d[2] == 255]
        mx, my, _ = tops[len(tops) // 2]
        m = np.full(gray.shape, 255, np.uint8)
        m[my, mx] = 0
        sc.mask = m
        sc.marks["masked_dot"] = (mx, my)
    return sc


COUNT_CLASSES = tuple(range(255, 175, -5))      # 16 brightness values, many buckets apart at the default quality level


def _count(n):
    pts = lattice(4, 4, 5, 17, 16, n)
    dots = with_brightness(pts, COUNT_CLASSES)
    runs = {"table5": dict(min_distance=5.0, **ONE_CELL), "accept_all": dict(min_distance=0.5, **ONE_CELL),
            "large70": dict(min_distance=70.0, **ONE_CELL)}
    if n == 257:
        runs["table5_harris"] = dict(min_distance=5.0, use_harris=1, **ONE_CELL)
        runs["max1"] = dict(max_corners=1, **ONE_CELL)
        runs["max1_large70"] = dict(max_corners=1, min_distance=70.0, **ONE_CELL)
    if n == 256:
        runs["quality1"] = dict(quality_level=1.0, **ONE_CELL)             # nothing exceeds the maximum: no candidate
    return Scene("count_%d" % n, dot_image(93, 88, dots), dots, runs)


TRIPLES = ((3, 4, 5), (6, 8, 10), (5, 12, 13))


def _radius_table():
    # pairs at distance exactly 5, 10 and 13 in four oblique orientations each and along both axes, every pair in a 40-px box of its
    # own: nothing but its partner within 13 px of a dot.  Brightness: equal within a pair (address decides) or not.
    dots, pairs = [], []
    k = 0
    for a, b, r in TRIPLES:
        for dx, dy in ((a, b), (b, a), (-a, b), (-b, a), (r, 0), (0, r)):
            bx, by = 20 + 40 * (k % 8), 20 + 40 * (k // 8)
            p, q = (bx, by), (bx + dx, by + dy)
            b0 = 255 - (k % 5)
            b1 = b0 if k % 2 == 0 else b0 - 7
            dots += [(p[0], p[1], b0), (q[0], q[1], b1)]
            pairs.append((p, q, r))
            k += 1
    runs = {}
    for _, _, r in TRIPLES:
        runs["r%d" % r] = dict(min_distance=float(r), **ONE_CELL)
        runs["r%d_up" % r] = dict(min_distance=up(r), **ONE_CELL)
    return Scene("radius_table_3_4_5", dot_image(340, 140, dots), dots, runs, marks={"pairs": pairs})


def _radius_64():
    # 17 x 16 dots at pitch 64: at 64.0 (the table kernel on the fused chain) all stay, at the next double (the grid kernel)
    # neighbours at distance exactly 64 conflict
    pts = lattice(5, 6, 64, 17, 16)
    dots = with_brightness(pts, (255, 240, 225, 210, 195, 180, 165))
    return Scene("radius_64", dot_image(1035, 973, dots), dots,
                 {"r64": dict(min_distance=64.0, **ONE_CELL), "r64_up": dict(min_distance=up(64.0), **ONE_CELL)})


PAIR_OFFSETS_65 = ((16, 63), (25, 60), (33, 56), (39, 52))      # dx^2 + dy^2 = 65^2


def _radius_65():
    # 17 x 16 dots at pitch 65, and below them four pairs at distance exactly 65 whose members lie in different grid cells (cell
    # = 65) in x and in y.  Order: pairs 0-2 take the six highest values (one 64-candidate step of the grid kernel); then 57
    # lattice dots; then pair 3, one member the last candidate of step 0, the other the first of step 1.
    lat = lattice(7, 9, 65, 17, 16)
    y_pairs = 9 + 65 * 15 + 75          # more than 65 below the lattice's last row
    dots, pairs = [], []
    for k, (dx, dy) in enumerate(PAIR_OFFSETS_65):
        p = (60 + 250 * k, y_pairs)      # the partner lies in the next cell column and row: checked on the CPU
        q = (p[0] + dx, p[1] + dy)
        pairs.append((p, q, 65))
    for k in range(3):
        dots += [(*pairs[k][0], 255 - 2 * k), (*pairs[k][1], 254 - 2 * k)]          # 255 .. 250
    dots += [(x, y, 245) for x, y in lat[:57]]
    dots += [(*pairs[3][0], 240), (*pairs[3][1], 235)]
    dots += with_brightness(lat[57:], (230, 215, 200, 185, 170))
    return Scene("radius_65", dot_image(1060, 1130, dots), dots,
                 {"r65": dict(min_distance=65.0, **ONE_CELL), "r65_up": dict(min_distance=up(65.0), **ONE_CELL)},
                 marks={"pairs": pairs})


def _ties(w):
    pts = lattice(3, 3, 6, 25, 20)
    dots = [(x, y, 200) for x, y in pts]
    runs = {"r6": dict(min_distance=6.0, **ONE_CELL), "r6_up": dict(min_distance=up(6.0), **ONE_CELL),
            "r13": dict(min_distance=13.0, **ONE_CELL),
            # at pitch 6 a radius of 13 reaches 12 neighbours, 6 of them of higher priority: within SUP_NB.  19 reaches 36 / 18.
            "r19": dict(min_distance=19.0, **ONE_CELL), "r6_up_harris": dict(min_distance=up(6.0), use_harris=1, **ONE_CELL)}
    return Scene("ties_500_w%d" % w, dot_image(w, 123, dots), dots, runs)


BORDER_SIZES = [(w, h) for w in (63, 64, 65) for h in (15, 16, 17, 65)]


def _border_ring(w, h):
    # dots on the two outermost rows and columns all the way round, alternating between them, at pitch 5, the corners, and one
    # dot in the middle; what is a candidate there (strictly interior pixels only) is the oracle's decision
    dots = {}
    for k, x in enumerate(range(5, w - 5, 5)):
        dots[(x, (0, 1)[k % 2])] = 255 - 3 * (k % 7)
        dots[(x, (h - 1, h - 2)[k % 2])] = 254 - 3 * (k % 7)
    for k, y in enumerate(range(5, h - 5, 5)):
        dots[((0, 1)[k % 2], y)] = 253 - 3 * (k % 7)
        dots[((w - 1, w - 2)[k % 2], y)] = 252 - 3 * (k % 7)
    for x, y in ((0, 0), (w - 2, 1), (1, h - 2), (w - 1, h - 1), (w // 2, h // 2)):
        dots.setdefault((x, y), 230)
    dl = [(x, y, b) for (x, y), b in sorted(dots.items(), key=lambda t: (t[0][1], t[0][0]))]
    runs = {"grid1x1": dict(**ONE_CELL), "grid5x3": dict(grid_rows=3, grid_cols=5)}
    return Scene("border_ring_%dx%d" % (w, h), dot_image(w, h, dl), dl, runs)


KEYPOINT_CLASSES = tuple(range(255, 127, -4))   # 32 values: 129 keys per value


def _keypoints(n):
    pts = lattice(3, 3, 5, 65, 64, n)
    dots = with_brightness(pts, KEYPOINT_CLASSES)
    runs = {"max0": dict(min_distance=0.0, max_corners=0, **ONE_CELL), "max4096": dict(min_distance=0.0, max_corners=4096, **ONE_CELL),
            "max5000": dict(min_distance=0.0, max_corners=5000, **ONE_CELL)}
    return Scene("keypoints_%d" % n, dot_image(331, 326, dots), dots, runs)


CAPACITY_FRAME = 256           # 256 x 256: the smallest keypoint buffer of a stage-level frame, 7168 (max(4096, w h / 16) * 1.5 + 1024)
CAPACITY = 7168


def _keypoint_capacity(n):
    # Dots at a pitch of 5 px give w h / 25 candidates at most, below any frame's keypoint capacity.  At pitch 4 equal
    # neighbours share a plateau between them and a dot yields about two candidates: 63 x 63 dots in nine bands of equal
    # brightness (seven rows each; about 440 keys per value) give 7317.  Leaving out the last 75 dots gives 7168, each further
    # one two less, and a lone dot in the space they leave one more.  The counts are the oracle's (test_gftt_edges_cpu.py).
    trim, lone = {7167: (76, True), 7168: (75, False), 7169: (75, True)}[n]
    pts = lattice(2, 2, 4, 63, 63)
    dots = [(x, y, 255 - 5 * (k // 63 // 7)) for k, (x, y) in enumerate(pts)][:63 * 63 - trim]
    if lone:
        dots.append((240, 250, 200))
    runs = {"max0": dict(min_distance=0.0, max_corners=0, **ONE_CELL), "max8000": dict(min_distance=0.0, max_corners=8000, **ONE_CELL),
            "max7168": dict(min_distance=0.0, max_corners=CAPACITY, **ONE_CELL), "max5000": dict(min_distance=0.0, max_corners=5000, **ONE_CELL)}
    return Scene("keypoint_capacity_%d" % n, dot_image(CAPACITY_FRAME, CAPACITY_FRAME, dots), dots, runs)


_BUILDERS = {
    "group_over_lds": _group_over_lds,
    "bucket_512": lambda: _bucket_edge("bucket_512", 512),
    "bucket_513": lambda: _bucket_edge("bucket_513", 513),
    "bucket_513_masked": lambda: _bucket_edge("bucket_513_masked", 513, masked=True),
    "count_1": lambda: _count(1),
    "count_255": lambda: _count(255),
    "count_256": lambda: _count(256),
    "count_257": lambda: _count(257),
    "radius_table_3_4_5": _radius_table,
    "radius_64": _radius_64,
    "radius_65": _radius_65,
    "ties_500_w156": lambda: _ties(156),       # w % 4 == 0
    "ties_500_w155": lambda: _ties(155),       # w % 4 == 3
    "keypoints_4095": lambda: _keypoints(4095),
    "keypoints_4096": lambda: _keypoints(4096),
    "keypoints_4097": lambda: _keypoints(4097),
    "keypoint_capacity_7167": lambda: _keypoint_capacity(7167),
    "keypoint_capacity_7168": lambda: _keypoint_capacity(7168),
    "keypoint_capacity_7169": lambda: _keypoint_capacity(7169),
}
for _w, _h in BORDER_SIZES:
    _BUILDERS["border_ring_%dx%d" % (_w, _h)] = functools.partial(_border_ring, _w, _h)

SCENE_NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name) -> Scene:
    return _BUILDERS[name]()


def cases():
    """every (scene name, run name)"""
    return [(n, r) for n in SCENE_NAMES for r in scene(n).runs]


def options(sc: Scene, run: str, module=oracle):
    """the run's options as the oracle's (module=oracle) or the library's (module=hip) structure"""
    return module.gftt_options(**sc.runs[run])


# ---- expectations (CPU oracle) ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(name, run):
    """-> (keypoints [n, 2] float32 in acceptance order, raw response map, candidate count): oracle.gftt, or the masked numpy
    reference for a scene with a detection mask (the oracle's detector has no mask argument)"""
    sc = scene(name)
    opt = options(sc, run)
    if sc.mask is not None:
        xy, eig, ncand = ref.gftt(sc.gray, opt, sc.mask)
    else:
        xy, _, ncand = oracle.gftt(sc.gray, opt, want_eig=True)     # (its map is the thresholded one)
        eig = ref.response(sc.gray, opt)
    for a in (xy, eig):
        a.setflags(write=False)
    return xy, eig, ncand


def ordered_candidates(sc: Scene, run: str):
    """-> (values float32 [n], x [n], y [n]) in processing order.  Unmasked: the oracle's own detector with min_distance 0
    and no limit, whose keypoints ARE the ordered candidates; masked: masked_gftt_ref.candidates"""
    opt = options(sc, run)
    eig = ref.response(sc.gray, opt)
    if sc.mask is not None:
        vals, idx = ref.candidates(eig, opt, sc.mask)
        return vals, (idx % sc.w).astype(np.int64), (idx // sc.w).astype(np.int64)
    opt.min_distance, opt.max_corners = 0.0, 0
    xy = oracle.gftt(sc.gray, opt).astype(np.int64)
    return eig[xy[:, 1], xy[:, 0]], xy[:, 0], xy[:, 1]


# ---- the sort's bucket rule, restated in integers -----------------------------------------------------------------------
def ordered_u32(v):
    """float_to_ordered (common.hpp): a monotone map of float32 onto uint32"""
    u = np.atleast_1d(np.asarray(v, np.float32)).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)


def sort_range(eig, opt, mask=None):
    """-> (hi, shift) of nms_kernel: hi = the largest per-cell maximum (over unmasked pixels; a cell without any counts as key
    0 and threshold 0.0), lo = the smallest per-cell threshold (float)(max * quality_level), clamped at 0.0, both as ordered
    keys; shift = the smallest with (hi - lo) >> shift < kSortBuckets (make_sort_range)"""
    h, w = eig.shape
    on = np.ones((h, w), bool) if mask is None else (np.asarray(mask) != 0)
    rows, cols = max(1, opt.grid_rows), max(1, opt.grid_cols)
    bh, bw = (h + rows - 1) // rows, (w + cols - 1) // cols
    hi, lo = 0, 0xffffffff
    for gy in range(rows):
        for gx in range(cols):
            cell, cell_on = eig[gy * bh:(gy + 1) * bh, gx * bw:(gx + 1) * bw], on[gy * bh:(gy + 1) * bh, gx * bw:(gx + 1) * bw]
            if cell.size and cell_on.any():
                mx = np.float32(cell[cell_on].max())
                key = int(ordered_u32(mx)[0])
            else:
                key, mx = 0, np.float32(0.0)       # no unmasked pixel (or a cell past the image): key 0, no positive threshold
            thr = np.float32(float(mx) * opt.quality_level)
            hi = max(hi, key)
            lo = min(lo, int(ordered_u32(thr if thr > 0 else np.float32(0.0))[0]))
    span = hi - lo if hi > lo else 0
    shift = 0
    while (span >> shift) >= SORT_BUCKETS:
        shift += 1
    return hi, shift


def buckets(vals, hi, shift):
    """bucket_of: bucket 0 holds the largest values"""
    d = np.maximum(hi - ordered_u32(vals), 0)
    return np.minimum(d >> shift, SORT_BUCKETS - 1)


def histogram(sc: Scene, run: str):
    """-> (bucket of every ordered candidate, bucket counts [kSortBuckets], group sums [kSortBuckets / 4], shift)"""
    opt = options(sc, run)
    vals, _, _ = ordered_candidates(sc, run)
    hi, shift = sort_range(ref.response(sc.gray, opt), opt, sc.mask)
    b = buckets(vals, hi, shift)
    hist = np.bincount(b, minlength=SORT_BUCKETS)
    return b, hist, hist.reshape(-1, BUCKETS_PER_WAVE).sum(1), shift


# ---- clips for the analyzer (tests/test_gftt_edges_product_gpu.py) ------------------------------------------------------------
CLIP_FLOW = dict(window_size=5, max_level=1)     # a small window and two levels: the CPU path of a clip stays within seconds


def rgb_of(gray):
    return np.ascontiguousarray(np.repeat(np.asarray(gray)[:, :, None], 3, axis=2))


def shifted(gray, dx):
    """the image moved dx pixels to the right (the scenes keep a margin of 3 px: nothing wraps)"""
    assert dx >= 0 and not gray[:, gray.shape[1] - dx:].any()
    return np.ascontiguousarray(np.roll(gray, dx, axis=1))


HINT_LEAD, HINT_EDGE_FRAMES = 12, 4
HINT_RUNS = {"default": {}, "accept_all": dict(min_distance=0.5), "large70": dict(min_distance=70.0)}


@functools.lru_cache(maxsize=None)
def hint_clip(n_edge):
    """12 frames of 64 dots -- the analyzer enqueues the first ten detections at full size, after them the launch hint sits at
    its floor of 4096 candidates -- then 4 frames of n_edge dots, every frame one pixel beside the previous one"""
    frames = []
    for t in range(HINT_LEAD + HINT_EDGE_FRAMES):
        ox = 3 + t % 2
        pts = lattice(ox + 30, 33, 35, 8, 8) if t < HINT_LEAD else lattice(ox, 3, 5, 65, 64, n_edge)
        frames.append(dot_image(332, 326, with_brightness(pts, KEYPOINT_CLASSES)))
    return frames


BUCKET_CLIP_GFTT = dict(quality_level=1e-20, **ONE_CELL)


@functools.lru_cache(maxsize=None)
def bucket_clip(first=512):
    """bucket_512 and bucket_513 in turns (the first frame: `first`), moved 0 / 1 / 2 px: every other frame overflows a value
    bucket"""
    return [shifted(scene("bucket_513" if (t + (first == 513)) % 2 else "bucket_512").gray, t % 3) for t in range(12)]


@functools.lru_cache(maxsize=None)
def ties_clip():
    return [shifted(scene("ties_500_w156").gray, t % 3) for t in range(12)]


def frame_histogram(gray, opt):
    """-> (candidate count, bucket counts) of one clip frame under the analyzer's options"""
    sc = Scene("clip_frame", gray, [], {"run": {k: getattr(opt, k) for k, _ in opt._fields_}})
    b, hist, groups, shift = histogram(sc, "run")
    return len(b), hist
