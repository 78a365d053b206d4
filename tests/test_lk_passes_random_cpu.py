"""CPU: the seeded cases of tests/lk_passes_cases.py alone, before any GPU is involved -- what the list covers is asserted on the
cases and on their REFERENCE (canonical arithmetic), so that tests/test_lk_passes_random_gpu.py compares the kernels with something
that exercises them.  Prints the coverage table, one line per case."""
import numpy as np
import pytest

import lk_affine_ref as aff_ref
import lk_passes_cases as K
import lk_search_ref as search_ref

WINDOWS = (3, 9, 10, 11, 16, 22, 31)
PASSES = ("search", "affine", "target_mask", "correlation", "fb", "window_mask")


def _cases(family=None):
    return [K.case(s) for s in K.SEEDS if family in (None, K.family_of(s))]


def test_the_list_holds_sixteen_seeds_per_family_and_a_case_is_deterministic():
    assert len(K.SEEDS) == 48 and all(sum(K.family_of(s) == f for s in K.SEEDS) == 16 for f in K.FAMILIES)
    K.case.cache_clear()
    a = K.case(27)
    K.case.cache_clear()
    b = K.case(27)
    assert a is not b and a.describe() == b.describe() and a.kps.tobytes() == b.kps.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.grays, b.grays))
    assert all((x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()) for x, y in zip(a.masks, b.masks))


@pytest.mark.parametrize("seed", K.SEEDS)
def test_case_stays_in_the_ranges_and_the_combinations_the_abi_accepts(seed):
    c = K.case(seed)
    assert 24 <= c.w < 260 and 24 <= c.h < 200 and 3 <= c.win <= 31 and 0 <= c.max_level <= 5 and 1 <= c.targets <= 8
    assert c.n * c.targets <= K.MAX_PAIRS and (c.n in K.N_CHOICES or c.n == K.MAX_PAIRS // c.targets)
    assert np.isfinite(c.kps).all() and c.kps.dtype == np.float32
    assert c.kps[:, 0].min(initial=0) >= -6 and c.kps[:, 0].max(initial=0) < c.w + 6
    assert c.kps[:, 1].min(initial=0) >= -6 and c.kps[:, 1].max(initial=0) < c.h + 6
    assert all(g.shape == (c.h, c.w) and g.dtype == np.uint8 for g in c.grays)
    assert c.min_correlation in K.MIN_CORRELATIONS and c.fb in K.FB_THRESHOLDS and c.margin in K.MARGINS
    if c.family == "constancy":
        assert c.R in K.RADII and (c.s, c.r) == search_ref.level_radius(c.R, c.T)
    else:       # normalize and mask_windows are refused beside a radius or the refinement, mask_windows beside a correlation too
        assert c.R == 0 and c.affine == 0
    if c.family == "window_masked":
        assert c.min_correlation == 0
    else:
        assert c.masks[0] is None
    if c.margin >= 0:
        assert c.masks[1] is not None, "a margin finds a masked target"
    if c.n >= 3:
        on_grid = (c.kps == np.floor(c.kps)).all(axis=1)
        assert on_grid[::3].all() and not on_grid.all()
    r = K.reference(c)
    for name in K.NAMES:
        lead = (c.n,) if name == "touched" else (c.targets, c.n)
        assert r[name].shape[:len(lead)] == lead, name


def test_keypoints_lie_on_both_sides_of_the_search_blocks_boundary():
    seen = 0
    for c in _cases("constancy"):
        if c.n < 23:
            continue
        ws, hs = c.levels[c.s]
        inside = [search_ref._inside(*search_ref.block_origin(x, y, c.s), ws, hs) for x, y in c.kps[[1, 7, 13, 19, 4, 10, 16, 22]]]
        assert inside == [True, False, False, True] * 2, (c.seed, inside)
        seen += 1
    assert seen >= 6


@pytest.mark.parametrize("family", K.FAMILIES)
def test_every_pinned_edge_occurs_in_the_family(family):
    cases = _cases(family)
    assert {c.win for c in cases} >= set(WINDOWS)
    assert {1, 8} <= {c.targets for c in cases} and {0, 1} <= {c.n for c in cases}
    assert any(c.max_level == 0 for c in cases)
    assert any(c.T < c.max_level for c in cases), "a pyramid that stops below max_level"
    assert any(c.levels[c.T][0] == c.win + 1 or c.levels[c.T][1] == c.win + 1 for c in cases), "a top level one pixel wider than the window"
    if family == "constancy":       # the search alone stages rows of a level as dwords
        live = [c for c in cases if c.n > 0]
        assert {c.levels[c.s][0] % 4 for c in live} >= {1, 2, 3}
        assert {c.R for c in cases} >= {5, 16, 17, 40, 100, 256}


def test_search_level_is_zero_intermediate_and_the_clamped_top_level():
    kinds = set()
    for c in _cases("constancy"):
        if c.n == 0:
            continue
        clamped = -(-c.R // (1 << c.s)) > search_ref.MAX_R
        assert not clamped or c.s == c.T
        kinds.add("clamped" if clamped else "zero" if c.s == 0 else "intermediate" if c.s < c.T else "top")
    assert kinds >= {"zero", "intermediate", "clamped"}, kinds


def test_every_state_occurs_and_no_pass_is_vacuous():
    sstate, astate, touched = np.zeros(3, int), np.zeros(3, int), np.zeros(2, int)
    acts = {p: [] for p in PASSES}
    print()
    for c in _cases():
        r = K.reference(c)
        ss, aa = np.bincount(r["search_state"].ravel(), minlength=3), np.bincount(r["affine_state"].ravel(), minlength=3)
        tt = np.bincount(r["touched"], minlength=2)
        sstate, astate, touched = sstate + ss, astate + aa, touched + tt
        print(c.describe(), "| search", ss.tolist(), "affine", aa.tolist(), "touched", tt.tolist(), "status 1:", int(r["status"].sum()))
        assert sorted(r["stages"]) == sorted(_passes_on(c)), (c.seed, sorted(r["stages"]))
        if c.n >= 63:
            for p, stage in r["stages"].items():
                acts[p].append((c.seed, K.pass_acts(p, stage)))
    assert sstate[search_ref.NONE] and sstate[search_ref.REPLACED] and sstate[search_ref.KEPT], sstate
    assert astate[aff_ref.ACCEPTED] and astate[aff_ref.UNCHANGED], astate
    assert touched[0] and touched[1], touched
    for p, seen in acts.items():
        both = [s for s, (changed, left) in seen if changed and left]
        print(p, "changes a row and leaves a row in", len(both), "of the", len(seen), "cases with n >= 63 that run it")
        assert len(seen) >= 3 and 4 * len(both) >= 3 * len(seen), (p, seen)


def _passes_on(c):
    on = []
    if c.family == "constancy":
        on.append("search")
        if c.affine:
            on.append("affine")
    if c.family == "window_masked" and c.masks[0] is not None:
        on.append("window_mask")
    if c.margin >= 0 and any(m is not None for m in c.masks[1:]):
        on.append("target_mask")
    if c.min_correlation > 0:
        on.append("correlation")
    if c.fb > 0:
        on.append("fb")
    return on


def test_x86_order_reference_is_a_second_reference_where_the_rule_has_two_instances():
    """the normalised rule has one; the other families' references differ between the modes in some row of the list (else the
    second comparison on the GPU would add nothing) and agree on what the mode plays no part in"""
    differ = {f: 0 for f in K.FAMILIES}
    for seed in (6, 12, 15, 7, 8, 14):
        c = K.case(seed)
        a, b = K.reference(c, "canonical"), K.reference(c, "x86")
        if c.family == "normalized":
            assert a is b
            continue
        assert a["search_d"].tobytes() == b["search_d"].tobytes() and a["touched"].tobytes() == b["touched"].tobytes()
        differ[c.family] += int((a["next_xy"].view(np.uint32) != b["next_xy"].view(np.uint32)).any(axis=2).sum())
    assert differ["constancy"] >= 1 and differ["window_masked"] >= 1, differ


@pytest.mark.parametrize("k", range(len(K.CLIP_SEEDS)))
def test_clip_evicts_frames_keeps_every_job_resident_and_finds_more_keypoints_with_time(k):
    clip = K.clip(k)
    nf = len(clip.rgb)
    assert 3 <= nf <= 9 and 1 <= clip.max_jobs <= 4 and 1 < clip.ring < nf, "the ring is smaller than the clip: frames are evicted"
    assert clip.case.family == K.FAMILIES[k // 4] and clip.log == (k % 2 == 0)
    assert [j[0] for j in clip.jobs] == list(range(clip.first, clip.first + nf))
    for f, (f1, tg) in enumerate(clip.jobs):       # the schedule of tests/test_lk_passes_random_gpu.py: frame f + 1 is put in front of job f
        put = min(f + 1, nf - 1)
        resident = set(range(clip.first + max(0, put - clip.ring + 1), clip.first + put + 1))
        assert tg and f1 not in tg and len(set(tg)) == len(tg) and set(tg) | {f1} <= resident, (f1, tg, sorted(resident))
    assert all(a < b for a, b in zip(clip.counts[:-2], clip.counts[2:])), "unmasked and unlimited, every frame holds more corners than the one two before it"
    assert clip.max_corners == 0 or min(clip.counts) < clip.max_corners <= max(clip.counts)
    assert all(f.shape == (clip.case.h, clip.case.w, 3) and (f[:, :, 0] == f[:, :, 1]).all() and (f[:, :, 1] == f[:, :, 2]).all() for f in clip.rgb)
