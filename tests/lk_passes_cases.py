"""Seeded cases of the passes behind the forward LK launch, and their reference.  TEST INFRASTRUCTURE ONLY.

case(seed) draws one LK job from np.random.default_rng(31000 + seed): the frame geometry (w in [24, 260), h in [24, 200), window
3..31, max_level 0..5, 1..8 targets, n keypoints from N_CHOICES capped to n * targets <= 400 -- the restatements cost some
milliseconds per (keypoint, target) pair, so a case's reference stays near two seconds), the images, the keypoints and the options
of its family:

    constancy       pc_lk_track_search: search radius, affine refinement, minimum correlation, forward-backward threshold, target-
                    side masks with a margin
    normalized      pc_lk_track_normalized: normalize 1 with the same correlation, threshold and margin draws
    window_masked   pc_lk_track_window_masked: mask_windows 1 with a mask on frame1 and on some targets, threshold and margin

The family is seed % 3.  The first len(PINNED) seeds of each family take their geometry from the written table PINNED, which pins
the edges a random draw meets too rarely; everything else of those seeds is drawn as for any other.

Images as in tests/lk_search_scene.py: frame1 is a crop of one fb_scene.texture canvas, a target a crop displaced beyond LK's
reach but within the search radius ('far'), by at most 3 px ('near'), by about half the reach ('half'), unrelated texture or a flat
plane; the normalized family puts some targets under lk_correlation_scene.gain.  Keypoints: uniform over [-6, w + 6) x [-6, h + 6),
a third of them on integer positions, and a few exactly on the inside / outside boundary of the search block (block origin 0 and
ws - 8 at the search level s).

reference(case, mode) chains oracle.lk (or the restatement's own forward rule) with the rules of tests/lk_*_ref.py and
tests/target_mask_ref.py in the order of run_lk_job (csrc/hip/api_lk.hip): masked windows | search, affine refinement, target-side
masks, minimum correlation, the backward pass.  It holds no arithmetic of its own."""
from __future__ import annotations

import functools

import numpy as np

import fb_scene
import lk_affine_ref as aff_ref
import lk_correlation_ref as corr_ref
import lk_correlation_scene
import lk_normalized_ref as norm_ref
import lk_search_ref as search_ref
import lk_window_mask_ref as wmask_ref
import oracle
import target_mask_ref as mask_ref

FAMILIES = ("constancy", "normalized", "window_masked")
N_CHOICES = (0, 1, 7, 63, 64, 65, 100, 257)
MAX_PAIRS = 400
RADII = (1, 5, 16, 17, 40, 100, 256)
MIN_CORRELATIONS = (0.0, 0.5, 0.75, 0.9)
FB_THRESHOLDS = (0.0, 0.5, 1.0, 2.0)
MARGINS = (-1, 0, 2, 7, 31)
KINDS = ("far", "near", "half", "unrelated", "flat")
PAD = 64          # the canvas reaches this far beyond frame1 on every side: the largest displacement of a target
NAMES = ("next_xy", "status", "err", "back_xy", "back_status", "affine_m", "affine_state", "search_d", "search_state", "touched")
MODES = ("canonical", "x86")

# The geometry of the first seeds of EVERY family (seed // 3 indexes the table).  Level widths: w_l = (w_{l-1} + 1) // 2, and the
# pyramid stops where the next level would not be wider and higher than the window.  With radius R the search level is the smallest s
# with ceil(R / 2^s) <= 16, clamped to the job's top level T (R and affine: constancy only, the other families ignore them).
PINNED = (
    # win 3, max_level 0; search level 0 is 101 wide: 101 = 1 (mod 4); 257 keypoints; one target
    dict(w=101, h=77, win=3, max_level=0, targets=1, n=257, R=5),
    # win 9; eight targets; R 40 -> s = 2 (< T = 3: an intermediate level), 150 -> 75 -> 38 wide: 38 = 2 (mod 4)
    dict(w=150, h=110, win=9, max_level=3, targets=8, n=257, R=40, affine=1),
    # win 10; R 100 -> s = 3, clamped to T = 2; 171 -> 86 -> 43 wide: 43 = 3 (mod 4)
    dict(w=171, h=96, win=10, max_level=2, targets=3, n=100, R=100, affine=1),
    # win 11, max_level 5 but the pyramid stops at level 2 (48 x 50, 24 x 25, 12 x 13; 6 x 7 is below the window), whose 12 columns
    # are one more than the window; R 256 -> s clamped to T = 2, where the 8 x 8 block has 5 x 6 positions
    dict(w=48, h=50, win=11, max_level=5, targets=2, n=63, R=256),
    # win 16; R 17 -> s = 1 of T = 2 (intermediate); odd sizes
    dict(w=133, h=89, win=16, max_level=2, targets=2, n=100, R=17, affine=1),
    # win 22 (two wavefronts per search workgroup), R 16: the largest radius matched at level 0
    dict(w=90, h=70, win=22, max_level=1, targets=4, n=64, R=16),
    # win 31 (one wavefront per search workgroup); 65 x 45 at level 1
    dict(w=130, h=90, win=31, max_level=1, targets=2, n=65, R=40, affine=1),
    # no keypoint at all
    dict(w=64, h=48, win=7, max_level=2, targets=5, n=0, R=16),
    # one keypoint, eight targets: one group of eight lanes in a wavefront holds a pair, per target
    dict(w=80, h=61, win=21, max_level=3, targets=8, n=1, R=40),
)
SEEDS = tuple(range(48))          # 16 per family, the first 9 of each pinned


def family_of(seed: int) -> str:
    return FAMILIES[seed % 3]


class Case:
    """one job: .seed .family .w .h .win .max_level .R .affine .min_correlation .fb .margin .kinds .grays [frame1, targets..]
    .masks [frame1's, targets'..] (None: no mask) .kps [n, 2] float32 .levels [(w_l, h_l)] .T .s .r"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n(self):
        return len(self.kps)

    @property
    def targets(self):
        return len(self.grays) - 1

    def flow_kw(self):
        return dict(window_size=self.win, max_level=self.max_level)

    def describe(self) -> str:
        widths = "/".join(str(w) for w, _ in self.levels)
        return (f"seed {self.seed:2d} {self.family:13s} {self.w:3d}x{self.h:3d} win {self.win:2d} L {self.max_level} T {self.T} widths {widths:15s} "
                f"targets {self.targets} n {self.n:3d} R {self.R:3d} s {self.s} r {self.r:2d} affine {self.affine} corr {self.min_correlation} "
                f"fb {self.fb} margin {self.margin:2d} masks {''.join('-' if m is None else 'm' for m in self.masks)} {','.join(self.kinds)}")


def _rect_mask(rng, w, h, value):
    """on (= value) but over a rectangle of a sixth to a third of each side, anywhere in the frame"""
    m = np.full((h, w), value, np.uint8)
    rw, rh = int(rng.integers(w // 6 + 1, w // 3 + 2)), int(rng.integers(h // 6 + 1, h // 3 + 2))
    rx, ry = int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))
    m[ry:ry + rh, rx:rx + rw] = 0
    return m


def _displacement(rng, magnitude):
    a = rng.uniform(0.0, 2.0 * np.pi)
    m = min(float(magnitude), float(PAD))
    dx, dy = int(round(m * np.cos(a))), int(round(m * np.sin(a)))
    return max(-PAD, min(PAD, dx)), max(-PAD, min(PAD, dy))


CACHED = 128          # cases and references kept: the 48 listed seeds and more, yet a soak over 10^5 seeds stays in memory


@functools.lru_cache(maxsize=CACHED)
def case(seed: int) -> Case:
    rng = np.random.default_rng(31000 + seed)
    family = family_of(seed)
    # ---- geometry: always drawn, so that a pinned seed's other draws do not depend on the table ----
    g = dict(w=int(rng.integers(24, 260)), h=int(rng.integers(24, 200)), win=int(rng.integers(3, 32)), max_level=int(rng.integers(0, 6)),
             targets=int(rng.integers(1, 9)), n=int(rng.choice(N_CHOICES)), R=int(rng.choice(RADII)))
    if seed // 3 < len(PINNED):
        g.update(PINNED[seed // 3])
    w, h, win, max_level, targets = g["w"], g["h"], g["win"], g["max_level"], g["targets"]
    n = min(g["n"], MAX_PAIRS // targets)
    levels = wmask_ref.level_sizes(w, h, win, max_level)
    T = len(levels) - 1
    # ---- options ----
    R = g["R"] if family == "constancy" else 0
    affine = int(rng.integers(0, 2))
    affine = g.get("affine", affine) if family == "constancy" else 0
    min_correlation = float(rng.choice(MIN_CORRELATIONS)) if family != "window_masked" else 0.0
    fb = float(rng.choice(FB_THRESHOLDS))
    margin = int(rng.choice(MARGINS))
    s, r = search_ref.level_radius(R, T) if R else (0, 0)
    # ---- images ----
    canvas = fb_scene.to_u8(fb_scene.texture(w + 2 * PAD, h + 2 * PAD, 100 + seed))

    def crop(dx=0, dy=0):
        return np.ascontiguousarray(canvas[PAD - dy:PAD - dy + h, PAD - dx:PAD - dx + w])

    reach = max(2, win // 2) << T                      # about what the pyramid lets LK follow
    far_hi = min(r << s if R else PAD, PAD, max(2, min(w, h) // 3))      # what the search reaches, and the frames still overlap
    mix = (0.3, 0.2, 0.2, 0.15, 0.15) if family == "constancy" else (0.1, 0.4, 0.3, 0.1, 0.1)
    kinds, grays = [], [crop()]
    for t in range(targets):
        kind = str(rng.choice(KINDS, p=mix))
        if t == 0:                                     # every job has a target in which its family's passes find work
            kind = "far" if family == "constancy" else "near"
        if kind == "far":
            lo = min(reach + 2, far_hi)
            gray = crop(*_displacement(rng, rng.uniform(lo, max(lo, 0.95 * far_hi))))
        elif kind == "near":
            gray = crop(int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
        elif kind == "half":
            gray = crop(*_displacement(rng, 0.5 * reach))
        elif kind == "unrelated":
            gray = fb_scene.to_u8(fb_scene.texture(w, h, 7000 + 10 * seed + t))
        else:
            gray = np.full((h, w), int(rng.integers(0, 256)), np.uint8)
        if family == "normalized" and kind not in ("flat",) and rng.random() < 0.5:
            gray = lk_correlation_scene.gain(gray, float(rng.choice([0.6, 0.8, 1.3])), float(rng.choice([-20.0, 15.0, 40.0])))
        kinds.append(kind)
        grays.append(gray)
    # ---- masks: frame1's is read by the masked windows alone, a target's by the margin test and the weighted backward pass ----
    masks = [None] * (1 + targets)
    if family == "window_masked" and (rng.random() < 0.85 or seed // 3 < len(PINNED)):      # (a pinned geometry always meets the rule)
        masks[0] = _rect_mask(rng, w, h, 255)
    want_target_masks = margin >= 0 or family == "window_masked"
    for t in range(targets):
        if want_target_masks and (rng.random() < 0.6 or (t == 0 and margin >= 0)):
            masks[1 + t] = _rect_mask(rng, w, h, 1 + 17 * t)
    # ---- keypoints ----
    kps = rng.uniform([-6.0, -6.0], [w + 6.0, h + 6.0], (n, 2)).astype(np.float32)
    kps[::3] = np.floor(kps[::3])
    ws, hs = levels[min(s, T)]
    scale = float(1 << s)
    edge_x = [3.5 * scale, np.nextafter(np.float32(3.5 * scale), np.float32(0)), (ws - 3.5) * scale, np.nextafter(np.float32((ws - 3.5) * scale), np.float32(0))]
    edge_y = [3.5 * scale, np.nextafter(np.float32(3.5 * scale), np.float32(0)), (hs - 3.5) * scale, np.nextafter(np.float32((hs - 3.5) * scale), np.float32(0))]
    if n >= 23:                                        # rows 1, 4, 7, ..: off the integer third
        for k in range(4):
            kps[1 + 6 * k] = (edge_x[k], rng.uniform(0.3 * h, 0.7 * h))
            kps[4 + 6 * k] = (rng.uniform(0.3 * w, 0.7 * w), edge_y[k])
    assert np.isfinite(kps).all()
    for a in grays + [m for m in masks if m is not None] + [kps]:
        a.setflags(write=False)
    return Case(seed=seed, family=family, w=w, h=h, win=win, max_level=max_level, R=R, affine=affine, min_correlation=min_correlation,
                fb=fb, margin=margin, kinds=kinds, grays=grays, masks=masks, kps=kps, levels=levels, T=T, s=s, r=r)


# ---- the reference ----
EMU = {"canonical": oracle.EMU_CANONICAL, "x86": oracle.EMU_OPENCV_X86}


@functools.lru_cache(maxsize=CACHED)
def _pyramids(seed: int):
    c = case(seed)
    with oracle.emulation(oracle.EMU_CANONICAL):      # the image and derivative planes do not depend on the LK order
        pyr = [oracle.Pyramid(np.array(g), c.win, c.max_level) for g in c.grays]
    assert [pyr[0].level_size(l) for l in range(pyr[0].num_levels)] == c.levels, (seed, c.levels)
    return pyr, [norm_ref.Planes(p) for p in pyr]


def _filters(c: Case, t: int, xy, st):
    """target-side masks, then minimum correlation: the status they leave"""
    if c.margin >= 0:
        st = mask_ref.keep(xy, st, c.masks[1 + t], c.margin)
    if c.min_correlation > 0:
        st, _ = corr_ref.rows(c.grays[0], c.grays[1 + t], c.win, c.kps, xy, st, c.min_correlation)
    return np.asarray(st, np.uint8)


def reference(c, mode: str = "canonical") -> dict:
    """c: a Case or its seed; mode: one of MODES (the normalised rule has one instance, which both modes must give)
    -> every array of the family's stage call, by name (NAMES): [targets, n, ..], touched [n]; zeros where the family has no such
    pass or the pass is off.  "stages" holds, per pass that ran, (status before, status after, rows the pass rewrote) for the
    coverage checks of tests/test_lk_passes_random_cpu.py.  Computed once per (seed, mode) and shared: the arrays are read-only."""
    seed = c.seed if isinstance(c, Case) else int(c)
    return _reference(seed, "canonical" if case(seed).family == "normalized" else mode)


@functools.lru_cache(maxsize=CACHED)
def _reference(seed: int, mode: str) -> dict:
    c = case(seed)
    n, nt = c.n, c.targets
    pyr, planes = _pyramids(seed)
    P, Ns = planes[0], planes[1:]
    opt = oracle.flow_options(**c.flow_kw())
    out = {"next_xy": np.zeros((nt, n, 2), np.float32), "status": np.zeros((nt, n), np.uint8), "err": np.zeros((nt, n), np.float32),
           "back_xy": np.zeros((nt, n, 2), np.float32), "back_status": np.zeros((nt, n), np.uint8),
           "affine_m": np.zeros((nt, n, 4), np.float32), "affine_state": np.zeros((nt, n), np.uint8),
           "search_d": np.zeros((nt, n, 2), np.int16), "search_state": np.zeros((nt, n), np.uint8), "touched": np.zeros(n, np.uint8)}
    stages = {}

    def note(name, before, after, rewrote=None):
        b, a, w = stages.setdefault(name, ([], [], []))
        b.append(np.array(before))
        a.append(np.array(after))
        w.append(np.zeros(n, bool) if rewrote is None else np.array(rewrote))

    if c.family == "constancy":
        with oracle.emulation(EMU[mode]):
            forward = [oracle.lk(pyr[0], pt, c.kps, opt) for pt in pyr[1:]]
        rows = search_ref.search(P, Ns, c.kps, forward, opt, c.R)
        for t in range(nt):
            note("search", forward[t][1], rows[t][1], rows[t][4] == search_ref.REPLACED)
        refined = aff_ref.refine(P, Ns, c.kps, [r[:3] for r in rows], opt) if c.affine else None
        for t in range(nt):
            xy, st, err, d, state = rows[t]
            if refined is not None:
                xy, st, err, m, astate = refined[t]
                out["affine_m"][t], out["affine_state"][t] = m, astate
                note("affine", st, st, astate == aff_ref.ACCEPTED)
            kept = _filters(c, t, xy, st)
            final, bxy, bst = kept, out["back_xy"][t], out["back_status"][t]
            if c.fb > 0:
                def plain_back(q, t=t):
                    with oracle.emulation(EMU[mode]):
                        b, sb, _ = oracle.lk(pyr[1 + t], pyr[0], q, opt)
                    return b, sb
                final, bxy, bst = search_ref.backward(P, Ns[t], c.kps, (xy, kept, err, d, state), opt, c.fb, plain_back)
                note("fb", kept, final)
            _store(out, t, xy, final, err, bxy, bst)
            out["search_d"][t], out["search_state"][t] = d, state
            _note_filters(c, t, note, xy, st, kept)
    elif c.family == "normalized":
        for t in range(nt):
            xy, st, err = norm_ref.track(P, Ns[t], c.kps, opt, normalize=True)
            kept = _filters(c, t, xy, st)
            final, bxy, bst = kept, out["back_xy"][t], out["back_status"][t]
            if c.fb > 0:
                _, final, _, bxy, bst = norm_ref.forward_backward(P, Ns[t], c.kps, opt, c.fb, True, forward=(xy, kept, err))
                note("fb", kept, final)
            _store(out, t, xy, final, err, bxy, bst)
            _note_filters(c, t, note, xy, st, kept)
    else:
        x86 = mode == "x86"
        weights = [None if m is None else wmask_ref.weight_pyramid(m, c.win, c.levels) for m in c.masks]
        for t in range(nt):
            xy, st, err, touched = wmask_ref.track(P, Ns[t], c.kps, opt, weights=weights[0], x86=x86)
            assert t == 0 or np.array_equal(touched, out["touched"]), "touched depends on frame1 and the keypoint alone"
            out["touched"] = touched
            kept = _filters(c, t, xy, st)
            final, bxy, bst = kept, out["back_xy"][t], out["back_status"][t]
            if c.fb > 0:
                _, final, _, bxy, bst = wmask_ref.forward_backward(P, Ns[t], c.kps, opt, c.fb, weights[0], weights[1 + t], x86=x86,
                                                                    forward=(xy, kept, err))
                note("fb", kept, final)
            _store(out, t, xy, final, err, bxy, bst)
            _note_filters(c, t, note, xy, st, kept)
        if weights[0] is not None:
            stages["window_mask"] = ([np.ones(n, np.uint8)], [np.ones(n, np.uint8)], [out["touched"] == 1])
    for a in out.values():
        a.setflags(write=False)
    out["stages"] = stages
    return out


def _store(out, t, xy, st, err, bxy, bst):
    out["next_xy"][t], out["status"][t], out["err"][t], out["back_xy"][t], out["back_status"][t] = xy, st, err, bxy, bst


def _note_filters(c, t, note, xy, st, kept):
    if c.margin >= 0 and c.masks[1 + t] is not None:
        note("target_mask", st, mask_ref.keep(xy, st, c.masks[1 + t], c.margin))
    if c.min_correlation > 0:
        before = mask_ref.keep(xy, st, c.masks[1 + t], c.margin) if c.margin >= 0 else st
        note("correlation", before, kept)


def pass_acts(name: str, stage) -> tuple:
    """(the pass changed a row, the pass left a row as it was) over all targets of a case; a row counts where the pass looks at it:
    status 1 in front of the pass, and for the search, which also rescues rows, every row"""
    before, after, rewrote = (np.concatenate(x) if len(x) else np.zeros(0) for x in stage)
    changed = (before != after) | rewrote.astype(bool)
    looked = np.ones(len(before), bool) if name == "search" else (before == 1) | changed
    return bool(changed.any()), bool((looked & ~changed).any())


# ---- clips for the analyzer ----
CLIP_SEEDS = (3, 12, 18, 33, 4, 28, 31, 46, 5, 17, 35, 41)      # the geometry and the options of these cases, four per family


class Clip:
    """.case (geometry and options) .first (id of frame 0) .rgb [frames] (R = G = B) .masks [per frame, None: put without one]
    .max_corners .ring .max_jobs .jobs [(frame1 id, [target ids])] in submission order .log (attach a device log)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def clip(k: int) -> Clip:
    """clip k of len(CLIP_SEEDS): 3..9 frames panning over one canvas -- by a step the search prepass is there for in the constancy
    family, by at most 2 px else -- whose right part is flat, less of it with every frame, so that the detector finds more
    keypoints from frame to frame and the buffers of a job lane grow inside the clip.  A job reads frame1 and up to `ring - 1`
    resident neighbours; frame f + 1 is put before job f is submitted, which evicts a frame while earlier jobs are in flight."""
    c = case(CLIP_SEEDS[k])
    rng = np.random.default_rng(32000 + k)
    nf = int(rng.integers(3, 10))
    first = int(rng.integers(1, 30))
    ring = int(min(nf - 1, rng.integers(2, 6)))
    max_jobs = 1 + (k + k // 4) % 4                    # 1..4, each with every family
    step = int(rng.integers(6, 13)) if c.family == "constancy" else int(rng.integers(0, 3))
    step_y = int(rng.integers(-2, 3))
    assert step * (nf - 1) <= 2 * PAD and 2 * (nf - 1) <= PAD
    canvas = fb_scene.to_u8(fb_scene.texture(c.w + 2 * PAD, c.h + 2 * PAD, 500 + k))
    rgb, masks, counts = [], [], []
    for t in range(nf):
        ox, oy = PAD + step * t - step * (nf - 1) // 2, PAD + step_y * t
        g = np.ascontiguousarray(canvas[oy:oy + c.h, ox:ox + c.w])
        g[:, int(c.w * (0.5 + 0.5 * t / (nf - 1))):] = 128
        with oracle.emulation(oracle.EMU_CANONICAL):
            counts.append(len(oracle.gftt(g)))
        rgb.append(np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)))
        masked = (c.family == "window_masked" or c.margin >= 0) and rng.random() < 0.7
        masks.append(_rect_mask(rng, c.w, c.h, 255) if masked else None)
    # some frames reach max_corners, some stay below: the counts differ from frame to frame
    max_corners = 0 if rng.random() < 0.3 else int(rng.integers((min(counts) + max(counts)) // 2, max(counts) + 1))
    jobs = []
    for f in range(nf):
        hi = min(f + 1, nf - 1)
        others = [x for x in range(max(0, hi - ring + 1), hi + 1) if x != f]
        take = rng.random(len(others)) < 0.7
        if not take.any():
            take[int(rng.integers(0, len(others)))] = True
        jobs.append((first + f, [first + x for x, on in zip(others, take) if on]))
    for a in rgb + [m for m in masks if m is not None]:
        a.setflags(write=False)
    return Clip(case=c, first=first, rgb=rgb, masks=masks, max_corners=max_corners, ring=ring, max_jobs=max_jobs, jobs=jobs, log=k % 2 == 0,
                counts=counts)
