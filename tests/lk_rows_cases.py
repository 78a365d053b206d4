"""Cases with a DICTATED status pattern for the small kernels every flow row passes through (csrc/hip/kernels_lk.hip: spatial
binning, ordered compaction, unpack_records_kernel, copy_keypoints_kernel), and their reference.  TEST INFRASTRUCTURE ONLY.

How the pattern is dictated.  Target-side masks with margin 0 judge a row by the pixel its end point rounds to
(tests/target_mask_ref.py).  Here frame1 is a 3 x 3 box blur of seeded uniform noise, target t is frame1 plus seeded integers in
[-3, 3], and a keypoint is an integer pixel at least win + 3 from the border: on the CPU oracle every such row has status 1, ends
within 0.07 px of its keypoint (the rounding limit is 0.5 px) and carries one of about two thousand distinct err values -- so the
mask byte at the keypoint's pixel IS the row's status, and a row that lands under the wrong index is seen by its err.  That is a
condition tests/test_lk_rows_cpu.py asserts for every case in both arithmetic orders, not an assumption.  mask_t[y_i, x_i] =
255 where pattern_t(i) holds, else 0; every other byte of the plane is seeded noise.  A pattern written "all*" is "all" on a
target that carries no mask (None), so masked and unmasked targets mix within a job.

A case is (win, n, keypoint order, pattern per target); frames are 192 x 128 with max_level 1, windows 10 (two keypoints per
wavefront of the LK kernel) and 11 (one).  Keypoint orders: "perm" a seeded permutation of the interior pixels (visiting order
and index order unrelated), "raster" ascending (y, x), "tile0" every keypoint inside the 64 x 64 tile (0, 0), "far" a permutation
with out-of-frame points of lk_subpixel_scene.FAR (scaled to this frame) spliced in at FAR_AT: their template window fails the
oracle's bounds test, so their expected status is the oracle's 0 whatever the mask says.

GEOMETRIES are the two frame sizes at the edge of bin_scan_kernel (256 tiles: one per lane; 272: two per lane, lanes 136.. own
none), with a few hundred keypoints in the first tile, the last tile and both tiles of one lane's pair.

rows() restates pc_lk_track_filtered from include/polychase_hip.h: per target the rows with status 1, ascending keypoint index,
targets back to back, row_offset[t] the first row of target t and row_offset[n_targets] the total."""
from __future__ import annotations

import functools

import numpy as np
from scipy.ndimage import uniform_filter

import oracle
import target_mask_ref as mask_ref

W, H, MAX_LEVEL = 192, 128, 1
WINDOWS = (10, 11)
AMPLITUDE = 3
MAX_TARGETS = 8
MODES = ("canonical", "x86")
EMU = {"canonical": oracle.EMU_CANONICAL, "x86": oracle.EMU_OPENCV_X86}      # EMU_OPENCV_X86 is the oracle's default
N_EDGES = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 511, 512, 513, 8191, 8192, 8193, 8449)
TOTALS = {255: (51, 5), 256: (32, 8), 259: (37, 7), 264: (33, 8), 272: (34, 8)}      # nblocks x n_targets

PATTERNS = {
    "all": lambda i, n, rng: np.ones(n, bool),
    "none": lambda i, n, rng: np.zeros(n, bool),
    "even": lambda i, n, rng: i % 2 == 0,
    "odd": lambda i, n, rng: i % 2 == 1,
    "m8": lambda i, n, rng: i % 8 == 0,
    "m32": lambda i, n, rng: i % 32 == 31,
    "b0": lambda i, n, rng: i % 256 == 0,
    "b255": lambda i, n, rng: i % 256 == 255,
    "blk2": lambda i, n, rng: (i // 256) % 2 == 0,
    "not0": lambda i, n, rng: i >= 256,                 # every block but block 0
    "first": lambda i, n, rng: i == 0,
    "last": lambda i, n, rng: i == n - 1,
    "r50": lambda i, n, rng: rng.random(n) < 0.5,
    "r02": lambda i, n, rng: rng.random(n) < 0.02,
}

# (win, n, keypoint order, pattern per target).  n_targets is the number of patterns.
TABLE = (
    (10, 1, "perm", "all"),
    (11, 1, "perm", "none"),
    (10, 1, "perm", "all*"),
    (10, 7, "perm", "first last"),
    (11, 8, "perm", "last odd even"),
    (10, 9, "perm", "m8 all* none first"),
    (11, 31, "perm", "m8 odd"),
    (10, 32, "perm", "m32 none all"),
    (11, 33, "perm", "m32 r50 even m8 none"),
    (10, 255, "perm", "b255 b0 r02 last all* r50"),
    (11, 256, "perm", "even b255 none odd b0 all first"),
    (10, 257, "perm", "b0 not0 blk2"),
    (10, 257, "far", "all* all all*"),
    (11, 511, "raster", "blk2 m8"),
    (10, 512, "raster", "not0 none r02 blk2"),
    (11, 513, "perm", "r02 last not0 b255 m32"),
    (10, 513, "perm", "odd"),
    (10, 2601, "tile0", "all r50 m32 not0"),
    (10, 8191, "perm", "r50 b0 none odd not0 b255"),
    (11, 8192, "perm", "all* none odd m8 m32 b255 blk2 r02"),        # 32 blocks x 8 = 256 counters
    (10, 8193, "perm", "last all* r50 none not0 b0 even first"),     # 33 x 8 = 264
    (11, 8193, "perm", "blk2"),
    (10, 8193, "far", "all all* all all* all all all* all"),
    (11, 8193, "far", "all* all all all* all all* all all"),
    (10, 8449, "perm", "none all r02 m8 odd m32 b255 b0"),           # 34 x 8 = 272
    (11, 9300, "perm", "b255 all* last blk2 odd none r02"),          # 37 x 7 = 259
    (11, 13000, "perm", "not0 first none r50 b0"),                   # 51 x 5 = 255
)
# keypoint indices that take a far point in a "far" case (dropped where >= n): the first and last keypoint of a wavefront's 8, of a
# 32-keypoint pass, of a block, and of the job
FAR_AT = (0, 7, 8, 31, 32, 255, 256, 8191, 8192)
# name: (w, h, tiles the keypoints occupy): first, both of lane 100's pair under two tiles per lane, last
GEOMETRIES = {"256 tiles": (1024, 1024, (0, 200, 201, 255)), "272 tiles": (1088, 1024, (0, 200, 201, 271))}
GEOMETRY_N, GEOMETRY_TARGETS = 300, (1, 3)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def images(w: int = W, h: int = H):
    """-> frame1, the eight targets (uint8 [h, w]): shared, read-only"""
    noise = np.random.default_rng(41000).integers(0, 256, (h, w)).astype(np.float64)
    f1 = np.rint(uniform_filter(noise, 3, mode="reflect")).astype(np.uint8)
    targets = [np.clip(f1.astype(np.int16) + np.random.default_rng(41100 + t).integers(-AMPLITUDE, AMPLITUDE + 1, (h, w)), 0, 255).astype(np.uint8)
               for t in range(MAX_TARGETS)]
    return _frozen(f1, *targets)[0], targets


def rgb(gray: np.ndarray) -> np.ndarray:
    """the gray image as the RGB frame the analyzer takes: rgb2gray gives it back"""
    return np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))


def interior(win: int, w: int = W, h: int = H) -> np.ndarray:
    """the integer pixels a keypoint may sit on, raster order, int64 [m, 2] (x, y)"""
    xs, ys = np.meshgrid(np.arange(win + 3, w - win - 3), np.arange(win + 3, h - win - 3))
    return np.stack([xs.ravel(), ys.ravel()], axis=1)


def far_points(w: int = W, h: int = H) -> np.ndarray:
    """the out-of-frame kinds of lk_subpixel_scene.FAR, written for a w x h frame: the template window fails the bounds test"""
    return np.array([(-1e6, 40.3), (50.7, 1e6), (1e6, 1e6), (-300.5, -200.25), (3 * w + 0.4, 10.1), (20.2, -2 * h - 0.6)], np.float32)


class Case:
    """.name .win .n .order .patterns [names, '*' stripped] .w .h .kps float32 [n, 2] .far bool [n] (out-of-frame rows) .want bool
    [n_targets, n] (the dictated pattern) .masks [per target: uint8 [h, w] or None] .grays [frame1, targets..]"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_targets(self):
        return len(self.patterns)

    @property
    def all_ones(self):
        return all(p == "all" for p in self.patterns)


def _keypoints(rng, win, n, order, w=W, h=H):
    px = interior(win, w, h)
    if order == "raster":
        px = px[np.sort(rng.choice(len(px), n, replace=False))]
    elif order == "tile0":
        px = px[(px[:, 0] < 64) & (px[:, 1] < 64)]
        px = px[rng.permutation(len(px))[:n]]
    else:
        px = px[rng.permutation(len(px))[:n]]
    assert len(px) == n, (order, n, len(px))
    kps, far = px.astype(np.float32), np.zeros(n, bool)
    if order == "far":
        pts = far_points(w, h)
        for k, i in enumerate(i for i in FAR_AT if i < n):
            kps[i], far[i] = pts[k % len(pts)], True
    return kps, far


def _make(name, seed, win, n, order, patterns, w=W, h=H, kps=None):
    rng = np.random.default_rng(42000 + seed)
    far = np.zeros(n, bool)
    if kps is None:
        kps, far = _keypoints(rng, win, n, order, w, h)
    f1, targets = images(w, h)
    i = np.arange(n)
    want, masks, names = np.zeros((len(patterns), n), bool), [], []
    for t, p in enumerate(patterns):
        unmasked = p.endswith("*")
        p = p.rstrip("*")
        assert p in PATTERNS and (not unmasked or p == "all"), p
        want[t] = PATTERNS[p](i, n, rng)
        m = None
        if not unmasked:
            m = rng.integers(0, 256, (h, w)).astype(np.uint8)
            ok = ~far
            m[kps[ok, 1].astype(int), kps[ok, 0].astype(int)] = np.where(want[t][ok], 255, 0)
        masks.append(m)
        names.append(p)
    _frozen(kps, far, want, *masks)
    return Case(name=name, seed=seed, win=win, n=n, order=order, patterns=names, w=w, h=h, kps=kps, far=far, want=want, masks=masks,
                grays=[f1] + targets[:len(patterns)])


NAMES = tuple("%02d-w%d-n%d-%s-t%d" % (k, win, n, order, len(p.split())) for k, (win, n, order, p) in enumerate(TABLE))
assert len(set(NAMES)) == len(NAMES)
GEOMETRY_NAMES = tuple("%s-%d" % (g, t) for g in GEOMETRIES for t in GEOMETRY_TARGETS)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    if name in GEOMETRY_NAMES:
        return _geometry_case(name)
    k = NAMES.index(name)
    win, n, order, p = TABLE[k]
    return _make(name, k, win, n, order, p.split())


def _geometry_case(name: str) -> Case:
    g, nt = name.rsplit("-", 1)
    w, h, tiles = GEOMETRIES[g]
    k = GEOMETRY_NAMES.index(name)
    rng = np.random.default_rng(43000 + k)
    px = interior(10, w, h)
    tile = (px[:, 1] >> 6) * ((w + 63) >> 6) + (px[:, 0] >> 6)
    px = px[np.isin(tile, tiles)]
    kps = px[rng.permutation(len(px))[:GEOMETRY_N]].astype(np.float32)
    return _make(name, 100 + k, 10, GEOMETRY_N, "perm", ("all*", "r50", "all*")[:int(nt)], w, h, kps)


def expected_status(c: Case, oracle_status: np.ndarray) -> np.ndarray:
    """the dictated pattern; the oracle's status on the out-of-frame rows, which have no mask byte"""
    return np.where(c.far[None, :], oracle_status, c.want).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference(name: str, mode: str):
    """-> (next_xy [T, n, 2], status [T, n], err [T, n], masked status [T, n]): oracle.lk per target in the mode's arithmetic,
    and its status under the target's mask with margin 0 (target_mask_ref.keep); computed once and shared, read-only"""
    c = case(name)
    opt = oracle.flow_options(window_size=c.win, max_level=MAX_LEVEL)
    nt = c.n_targets
    xy, st, err = np.zeros((nt, c.n, 2), np.float32), np.zeros((nt, c.n), np.uint8), np.zeros((nt, c.n), np.float32)
    kept = np.zeros((nt, c.n), np.uint8)
    with oracle.emulation(EMU[mode]):
        p1 = oracle.Pyramid(np.array(c.grays[0]), c.win, MAX_LEVEL)
        for t in range(nt):
            xy[t], st[t], err[t] = oracle.lk(p1, oracle.Pyramid(np.array(c.grays[1 + t]), c.win, MAX_LEVEL), c.kps, opt)
            kept[t] = mask_ref.keep(xy[t], st[t], c.masks[t], 0)
    return _frozen(xy, st, err, kept)


def rows(status: np.ndarray, xy: np.ndarray, err: np.ndarray):
    """status [T, n], xy [T, n, 2], err [T, n] -> (row_offset int64 [T + 1], idx uint32 [M], xy float32 [M, 2], err float32 [M])"""
    status = np.asarray(status)
    keep = [np.nonzero(status[t] == 1)[0] for t in range(len(status))]
    off = np.zeros(len(status) + 1, np.int64)
    off[1:] = np.cumsum([len(k) for k in keep])
    if not len(keep):
        return off, np.zeros(0, np.uint32), np.zeros((0, 2), np.float32), np.zeros(0, np.float32)
    return (off, np.concatenate(keep).astype(np.uint32), np.concatenate([xy[t][k] for t, k in enumerate(keep)]).astype(np.float32).reshape(-1, 2),
            np.concatenate([err[t][k] for t, k in enumerate(keep)]).astype(np.float32))


def split_rows(r):
    """rows() -> per target (idx, xy, err), the form hip.lk_track_filtered and Analyzer.collect return"""
    off, idx, xy, err = r
    return [(idx[a:b], xy[a:b], err[a:b]) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


# ---- jobs of the analyzer's lane sequences ----
# what each of the two lanes sees, in this order (job j runs on lane j & 1: jobs 2 k and 2 k + 1 take entry k)
LANE_SEQUENCE = ((8193, 8), (1, 1), (257, 3), (0, 2), (8193, 8), (512, 0), (513, 5))
SEQUENCE_WIN = {1: 10, 2: 11, 3: 10}          # window by max_jobs
# The jobs of a sequence share the eight target frames, so a target's mask is ONE plane for all of them: bytes that are non-zero with
# this probability (None: the target carries no mask).  A job's pattern is its own keypoints read through these planes -- dictated
# all the same, and different from job to job because every job draws its own keypoints.
SEQUENCE_MASKS = (0.5, None, 0.02, 0.0, 0.5, 0.98, None, 0.25)


@functools.lru_cache(maxsize=None)
def sequence_jobs(max_jobs: int):
    """-> [Case] in submission order: job j has LANE_SEQUENCE[j // 2]'s (n, n_targets) and its own seeded permutation of the interior
    pixels; it reads targets 0 .. n_targets - 1 of images() under the sequence's masks (every Case holds the same planes)"""
    win = SEQUENCE_WIN[max_jobs]
    rng = np.random.default_rng(44000 + max_jobs)
    f1, targets = images()
    masks = [None if p is None else np.where(rng.random((H, W)) < p, rng.integers(1, 256, (H, W)), 0).astype(np.uint8) for p in SEQUENCE_MASKS]
    _frozen(*masks)
    jobs = []
    for j in range(2 * len(LANE_SEQUENCE)):
        n, nt = LANE_SEQUENCE[j // 2]
        kps, far = _keypoints(rng, win, n, "perm")
        x, y = kps[:, 0].astype(int), kps[:, 1].astype(int)
        want = np.array([np.ones(n, bool) if m is None else m[y, x] != 0 for m in masks[:nt]], bool).reshape(nt, n)
        _frozen(kps, far, want)
        jobs.append(Case(name="job %d" % j, seed=j, win=win, n=n, order="perm", patterns=["p=%s" % p for p in SEQUENCE_MASKS[:nt]], w=W, h=H,
                         kps=kps, far=far, want=want, masks=masks[:nt], grays=[f1] + targets[:nt]))
    return jobs
