"""CPU: the cases of tests/lk_rows_cases.py alone, before any GPU is involved.

  * the status pattern IS dictated: on the oracle, in canonical arithmetic and in its default (x86) emulation, every in-frame row of
    every case has status 1 and ends on its keypoint's pixel, so oracle.lk filtered by target_mask_ref.keep(margin 0) is the
    pattern; the out-of-frame rows have status 0;
  * the list covers the edges it was written for (the table is printed);
  * comparing with rows() has teeth: a numpy model of the two-launch compaction (kernels_lk.hip: compact_count_kernel with
    compact_scan_body in its tail, compact_scatter_kernel) equals rows() on every case, and each of six defects, switched on alone,
    changes the output of at least one case."""
import numpy as np
import pytest

import lk_rows_cases as K
import target_mask_ref as mask_ref

# literals, not imports: each mirrors a constant of the kernels
BLOCK = 256          # kernels_lk.hip CF: keypoints per compaction workgroup
PASS = 32            # kernels_lk.hip CT / kRecStride: keypoints a workgroup walks per pass
WAVE = 8             # 64 / kRecStride: keypoints of one wavefront within a pass
TICKET_GROUP = 32    # common.hpp kTicketGroup: workgroups per ticket word
SCAN_LANES = 256     # kernels_lk.hip compact_scan_body: lanes that share the counters
SLOTS = 8            # kRecStride: records per keypoint slot of a lane, one per target
TILE_SHIFT = 6       # kernels_lk.hip BIN_SHIFT


def geometry(n, nt):
    nblocks = -(-n // BLOCK)
    total = nblocks * nt
    per = -(-total // SCAN_LANES)
    groups = -(-nblocks // TICKET_GROUP)
    return dict(nblocks=nblocks, total=total, per=per, groups=groups, last_group=nblocks - TICKET_GROUP * (groups - 1) if groups else 0,
                idle_last_lane=total > 0 and (SCAN_LANES - 1) * per >= total)


def block_counts(c):
    """rows per (target, block) of the dictated pattern"""
    st = K.expected_status(c, np.zeros((c.n_targets, c.n), np.uint8))
    nblocks = -(-c.n // BLOCK)
    pad = np.zeros((c.n_targets, nblocks * BLOCK), np.int64)
    pad[:, :c.n] = st
    return pad.reshape(c.n_targets, nblocks, BLOCK).sum(axis=2)


def _gap(v):
    """an empty entry between two non-empty ones"""
    nz = np.nonzero(np.asarray(v))[0]
    return len(nz) >= 2 and (np.asarray(v)[nz[0]:nz[-1]] == 0).any()


@pytest.mark.parametrize("name", K.NAMES + K.GEOMETRY_NAMES)
def test_the_pattern_is_dictated(name):
    c = K.case(name)
    assert c.kps.dtype == np.float32 and c.kps.shape == (c.n, 2) and len(c.masks) == c.n_targets <= K.MAX_TARGETS
    ok = ~c.far
    px = c.kps[ok].astype(np.int64)
    assert (px == c.kps[ok]).all() and len({(x, y) for x, y in px.tolist()}) == len(px), "distinct integer pixels"
    lo, hi = c.win + 3, (c.w - c.win - 3, c.h - c.win - 3)
    assert (px >= lo).all() and (px[:, 0] < hi[0]).all() and (px[:, 1] < hi[1]).all()
    for t, m in enumerate(c.masks):
        assert (m is None) == (c.patterns[t] == "all" and m is None)
        if m is not None:
            assert np.array_equal(m[px[:, 1], px[:, 0]] != 0, c.want[t][ok]) and 0 < (m == 0).sum() < m.size
    for mode in K.MODES:
        xy, st, err, kept = K.reference(name, mode)
        ix, iy = mask_ref.pixel(xy, c.w, c.h)
        for t in range(c.n_targets):
            assert (st[t][ok] == 1).all(), (name, mode, t, "a row is lost")
            assert (ix[t][ok] == px[:, 0]).all() and (iy[t][ok] == px[:, 1]).all(), (name, mode, t, "an end point leaves its pixel")
            assert (st[t][c.far] == 0).all() and (err[t][c.far] == 0).all(), (name, mode, t, "out-of-frame rows")
            assert np.array_equal(kept[t][ok] == 1, c.want[t][ok]), (name, mode, t)
            assert np.array_equal(kept[t], K.expected_status(c, st)[t]), (name, mode, t)
        if c.n >= 255:      # a swapped row shows: the err values are (nearly) all different
            assert len(np.unique(err[:, ok])) >= 0.5 * min(ok.sum(), 1000), (name, mode)


def test_the_list_covers_the_edges_it_was_written_for():
    cases = [K.case(name) for name in K.NAMES]
    assert 25 <= len(cases) <= 35
    print()
    seen = dict(gap_block=[], gap_target=[], empty_last=[], idle_last_lane=[], idle_with_two_per_lane=[], single_member_group=[])
    first, last = set(), set()
    for c in cases:
        g, cnt = geometry(c.n, c.n_targets), block_counts(c)
        per_target = cnt.sum(axis=1)
        print("%-22s win %2d n %5d targets %d blocks %2d counters %3d per %d ticket groups %d (last holds %2d) far %d | %s | rows per target %s"
              % (c.name, c.win, c.n, c.n_targets, g["nblocks"], g["total"], g["per"], g["groups"], g["last_group"], int(c.far.sum()),
                 " ".join(p + ("" if m is not None else "*") for p, m in zip(c.patterns, c.masks)), per_target.tolist()))
        if c.n <= 2601:
            print("%22s rows per (target, block): %s" % ("", cnt.tolist()))
        first.add(c.patterns[0])
        last.add(c.patterns[-1])
        if any(_gap(row) for row in cnt):
            seen["gap_block"].append(c.name)
        if _gap(per_target):
            seen["gap_target"].append(c.name)
        if c.n_targets >= 2 and per_target[-1] == 0 and per_target[:-1].any():
            seen["empty_last"].append(c.name)
        if g["idle_last_lane"]:
            seen["idle_last_lane"].append(c.name)
            if g["per"] >= 2:
                seen["idle_with_two_per_lane"].append(c.name)
        if g["groups"] == 2 and g["last_group"] == 1:
            seen["single_member_group"].append(c.name)
    for what, names in seen.items():
        print(what, names)
        assert names, what
    assert {c.n for c in cases} >= set(K.N_EDGES)
    have = {(geometry(c.n, c.n_targets)["nblocks"], c.n_targets) for c in cases}
    assert have >= set(K.TOTALS.values()) and all(b * t == total for total, (b, t) in K.TOTALS.items())
    assert all(sum(c.n_targets == t for c in cases) >= 2 for t in range(1, K.MAX_TARGETS + 1))
    assert first >= set(K.PATTERNS) and last >= set(K.PATTERNS), (set(K.PATTERNS) - first, set(K.PATTERNS) - last)
    assert any("none" in c.patterns[1:-1] for c in cases) and any(c.patterns[-1] == "none" and c.n_targets >= 2 for c in cases)
    assert {c.win for c in cases if c.order == "raster"} == set(K.WINDOWS)
    assert any(c.order == "tile0" and c.kps.max() < 64 for c in cases)
    assert {c.win for c in cases if c.order == "far"} == set(K.WINDOWS) and all(c.far.any() == (c.order == "far") for c in cases)
    assert any(any(m is None for m in c.masks) and any(m is not None for m in c.masks) for c in cases), "masked and unmasked targets in one job"
    # the order the filtered stage calls of tests/test_lk_rows_gpu.py need: all-ones or out-of-frame cases at these (n, n_targets)
    free = {(c.n, c.n_targets) for c in cases if c.all_ones}
    assert free >= {(8193, 8), (1, 1), (257, 3)}


def test_bin_scan_geometries_sit_at_one_and_two_tiles_per_lane():
    for name in K.GEOMETRY_NAMES:
        c = K.case(name)
        tiles_x, tiles_y = (c.w + 63) >> TILE_SHIFT, (c.h + 63) >> TILE_SHIFT
        n_tiles = tiles_x * tiles_y
        per = -(-n_tiles // SCAN_LANES)
        tile = (c.kps[:, 1].astype(int) >> TILE_SHIFT) * tiles_x + (c.kps[:, 0].astype(int) >> TILE_SHIFT)
        used = sorted(set(tile.tolist()))
        print(name, c.w, c.h, "tiles", n_tiles, "per lane", per, "occupied", used, np.bincount(tile)[used].tolist())
        assert n_tiles == int(name.split()[0]) and per == (1 if n_tiles == 256 else 2)
        assert used == sorted(K.GEOMETRIES[name.rsplit("-", 1)[0]][2]) and used[0] == 0 and used[-1] == n_tiles - 1
        assert used[1] % per == 0 and used[2] == used[1] + 1, "both tiles of one lane's pair"
        assert ((SCAN_LANES - 1) * per >= n_tiles) == (n_tiles == 272), "at 272 tiles lanes 136.. own nothing"
        assert 200 <= c.n <= 500 and len(used) < n_tiles // 16


def test_lane_sequences_reuse_a_lane_with_fewer_targets_and_fewer_blocks():
    for max_jobs in (1, 2, 3):
        jobs = K.sequence_jobs(max_jobs)
        assert len(jobs) >= 8 and [(c.n, c.n_targets) for c in jobs[0::2]] == list(K.LANE_SEQUENCE) == [(c.n, c.n_targets) for c in jobs[1::2]]
        assert all(a.want.tobytes() != b.want.tobytes() or a.n * a.n_targets == 0 for a, b in zip(jobs, jobs[2:]) if a.want.shape == b.want.shape)
        assert all(a.kps.tobytes() != b.kps.tobytes() for a, b in zip(jobs[0::2], jobs[1::2]) if a.n)
    seq = K.LANE_SEQUENCE
    assert any(a[1] == 8 and 0 < b[1] < 8 for a, b in zip(seq, seq[1:])), "records of eight targets under a job with fewer"
    assert (0, 2) in seq and any(nt == 0 and n > 0 for n, nt in seq)
    assert any(-(-a[0] // BLOCK) > -(-b[0] // BLOCK) > 0 for a, b in zip(seq, seq[1:])), "fewer blocks than the launch before"


# ---- a model of the two launches, with defects ----
DEFECTS = ("per_rounded_down", "total_from_idle_lane", "prefix_in_wave_pass_order", "tail_counted", "stale_targets_counted", "visiting_order")


def visiting_order(c):
    """slot_of [n]: counting sort by 64 x 64 tile, raster order of tiles, the tile index clamped (the order inside a tile is left to
    atomics on the GPU; the model takes the stable one)"""
    tiles_x, n_tiles = (c.w + 63) >> TILE_SHIFT, ((c.w + 63) >> TILE_SHIFT) * ((c.h + 63) >> TILE_SHIFT)
    x, y = c.kps[:, 0].astype(np.int32), c.kps[:, 1].astype(np.int32)
    tile = np.clip((y >> TILE_SHIFT).astype(np.int64) * tiles_x + (x >> TILE_SHIFT), 0, n_tiles - 1)
    perm = np.argsort(tile, kind="stable")
    slot_of = np.empty(c.n, np.int64)
    slot_of[perm] = np.arange(c.n)
    return slot_of, perm


def model(status, xy, err, slot_of, perm, defect=None):
    """-> (row_offset [T + 1], idx, xy, err) as the host reads them: buffers of T * n rows, row_offset zeroed before the launches.
    The lane's records lie in visiting order, SLOTS per keypoint; what this job does not write is STALE: status 1 and a marker,
    as an earlier, larger job with eight targets leaves them."""
    T, n = status.shape
    nblocks = -(-n // BLOCK)
    S = nblocks * BLOCK
    cap = T * n
    row_offset = np.zeros(T + 1, np.int64)
    out_idx, out_xy, out_err = np.full(cap, 0xFFFFFFFF, np.uint32), np.full((cap, 2), -2.0, np.float32), np.full(cap, -2.0, np.float32)
    if nblocks == 0 or T == 0:
        return row_offset, out_idx, out_xy, out_err
    rec_st, rec_xy, rec_err = np.ones((S, SLOTS), np.uint8), np.full((S, SLOTS, 2), -1.0, np.float32), np.full((S, SLOTS), -1.0, np.float32)
    rec_st[slot_of, :T], rec_xy[slot_of, :T], rec_err[slot_of, :T] = status.T, xy.transpose(1, 0, 2), err.T
    slot = np.arange(S)          # slot_of beyond n: stale too, some slot the job does not use
    index = np.arange(S)         # the keypoint index a lane emits
    if defect == "visiting_order":
        index[:n] = perm
    else:
        slot[:n] = slot_of
    live_n = S if defect == "tail_counted" else n
    live_t = SLOTS if defect == "stale_targets_counted" else T
    keep = (rec_st[slot] == 1) & (np.arange(S) < live_n)[:, None]          # [position, slot]
    # launch 1: counts per (target, block), published for the job's targets only; then the scan in the last workgroup
    counts = keep[:, :T].reshape(nblocks, BLOCK, T).sum(axis=1).T.reshape(-1).astype(np.int64)      # [t * nblocks + b]
    total = nblocks * T
    per = total // SCAN_LANES if defect == "per_rounded_down" else -(-total // SCAN_LANES)
    offsets = counts.copy()
    lane_run = np.zeros(SCAN_LANES, np.int64)       # a lane that owns nothing has left before the scan
    run = 0
    for lane in range(SCAN_LANES):
        b, e = lane * per, min(lane * per + per, total)
        for i in range(b, e):
            if i % nblocks == 0:
                row_offset[i // nblocks] = run
            offsets[i] = run
            run += counts[i]
        if b < e:
            lane_run[lane] = run
            if e == total and defect != "total_from_idle_lane":
                row_offset[T] = run
    if defect == "total_from_idle_lane":
        row_offset[T] = lane_run[SCAN_LANES - 1]
    # launch 2: per block, the rows of a target in keypoint order = (pass, wavefront) order
    local = np.arange(BLOCK)
    k, w, j = local // PASS, (local % PASS) // WAVE, local % WAVE
    order = np.lexsort((j, k, w)) if defect == "prefix_in_wave_pass_order" else np.lexsort((j, w, k))
    # (the lanes of a stale slot take base 0 and race with the job's own rows for the first positions of the buffers: any outcome of
    # a race may happen, the model takes the one that shows -- the stale row written last)
    for t in range(live_t):
        for b in range(nblocks):
            base = offsets[t * nblocks + b] if t < T else 0
            p = b * BLOCK + order[keep[b * BLOCK + order, t]]
            pos = base + np.arange(len(p))
            ok = pos < cap
            out_idx[pos[ok]], out_xy[pos[ok]], out_err[pos[ok]] = index[p[ok]], rec_xy[slot[p[ok]], t], rec_err[slot[p[ok]], t]
    return row_offset, out_idx, out_xy, out_err


def _same(got, want):
    off, idx, xy, err = want
    m = len(idx)
    return (np.array_equal(got[0], off) and got[1][:m].tobytes() == idx.tobytes() and got[2][:m].tobytes() == xy.tobytes()
            and got[3][:m].tobytes() == err.tobytes())


def test_the_model_equals_rows_and_every_defect_changes_some_case():
    caught = {d: [] for d in DEFECTS}
    for name in K.NAMES:
        c = K.case(name)
        xy, _, err, kept = K.reference(name, "canonical")
        want = K.rows(kept, xy, err)
        slot_of, perm = visiting_order(c)
        assert sorted(slot_of.tolist()) == list(range(c.n))
        assert _same(model(kept, xy, err, slot_of, perm), want), name
        for d in DEFECTS:
            if not _same(model(kept, xy, err, slot_of, perm, d), want):
                caught[d].append(name)
    print()
    for d, names in caught.items():
        print("%-26s changes %2d of %d cases: %s" % (d, len(names), len(K.NAMES), " ".join(names)))
    for d, names in caught.items():
        assert names, d
    by_total = {geometry(K.case(name).n, K.case(name).n_targets)["total"]: name for name in K.NAMES}
    # 256 counters: every lane owns one, so neither scan defect can show there; 264: two per lane and idle upper lanes, both show
    assert by_total[256] not in caught["per_rounded_down"] + caught["total_from_idle_lane"]
    assert by_total[264] in caught["per_rounded_down"] and by_total[264] in caught["total_from_idle_lane"]


def test_rows_is_the_header_s_rule_on_a_written_example():
    st = np.array([[1, 0, 1, 2], [0, 0, 0, 0], [0, 1, 0, 0]], np.uint8)
    xy = np.arange(24, dtype=np.float32).reshape(3, 4, 2)
    err = np.arange(12, dtype=np.float32).reshape(3, 4)
    off, idx, rxy, rerr = K.rows(st, xy, err)
    assert off.tolist() == [0, 2, 2, 3] and idx.tolist() == [0, 2, 1] and idx.dtype == np.uint32
    assert rxy.tolist() == [[0, 1], [4, 5], [18, 19]] and rerr.tolist() == [0, 2, 9]
    assert [len(r[0]) for r in K.split_rows((off, idx, rxy, rerr))] == [2, 0, 1]
    assert K.rows(np.zeros((0, 5), np.uint8), np.zeros((0, 5, 2), np.float32), np.zeros((0, 5), np.float32))[0].tolist() == [0]
