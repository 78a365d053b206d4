"""GPU: lens undistortion at ingest at the C ABI (pc_context_set_lens_map) -- frames put under a lens map through pc_frame_set_rgb /
_rgb_f32 / _gray against the numpy rule (tests/lens_ref.py) fed to the CPU oracle.  Everything is bit-exact; nothing is a tolerance.

  * tests/_lens_check.py has the case list and what a case compares (gray; per level the padded u8 plane, the derivative plane and
    the uint16 plane).  The cases run here on gray kernel -> remap -> fused level kernel (at 23 x 19 under a 25-px window on the
    unfused chain) and once more in ONE child process under POLYCHASE_PYRAMID_VARIANT=1;
  * an identity map gives the planes of a context that never set a map; clearing the map restores the planes AND the launches per
    timing class of such a context;
  * a frame of another size is refused and keeps its planes; a refused setter changes nothing;
  * pc_frame_detect and pc_lk_track on remapped frames equal oracle.gftt / oracle.lk on lens_ref's output: the lens acts before
    everything else."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ingest_check as check
import _lens_check as lc
import ingest_layouts as il
import lens_ref as ref
import oracle
from polychase_amd import hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PC_E_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


# ---- the cases, fused level kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.cases(), ids=lc.case_name)
def test_planes_under_a_lens_map_match_the_rule(ctx, case):
    assert os.environ.get("POLYCHASE_PYRAMID_VARIANT", "0") == "0", "this process must run the fused level kernel"
    assert lc.run_case(ctx, case) == ""


@pytest.mark.parametrize("extra", lc.EXTRA, ids=lc.extra_name)
def test_pinned_frames_and_gray_conversions_under_a_lens_map(ctx, extra):
    assert lc.run_extra(ctx, extra) == ""


def test_the_case_list_covers_what_it_claims():
    assert [(w % 4, w > 64) for w, _, _ in lc.SIZES[:4]] == [(3, False), (0, False), (1, True), (3, True)]
    assert (23, 19, 25) in lc.SIZES and not (23 > 25 + 1)                 # level_fits_fused is false there
    for w, h, win in lc.SIZES:
        q = lc.lens_map("random", w, h)
        assert set(np.unique(q[..., 0] & 255)) == set(range(256)) and set(np.unique(q[..., 1] & 255)) == set(range(256))
        assert q[..., 0].min() < 0 and q[..., 0].max() > (w - 1) * 256 and q[..., 1].min() < 0 and q[..., 1].max() > (h - 1) * 256
        assert q[..., 0].min() >= -3 * 256 and q[..., 0].max() <= (w + 2) * 256
        inv = lc.lens_map("invalid", w, h)
        bad = (inv == ref.INVALID).any(axis=2)
        assert bad.sum() >= 45 and (inv == ref.INVALID).all(axis=2).sum() < bad.sum()
        cl = lc.lens_map("clamped", w, h)
        assert (cl == ref.CLAMP).any() and (cl == -ref.CLAMP).any()
        pin = lc.lens_map("pincushion", w, h)
        assert (ref.valid(pin) == 0).any() and (ref.valid(pin) == 255).any()
        # the maps change the picture, each in its own way
        e = [lc.expected("rgb", w, h, win, 0, name).gray for name in lc.MAPS]
        assert np.array_equal(e[0], il.gray_of(check.image("rgb", w, h, 0)))
        assert len({a.tobytes() for a in e}) == len(lc.MAPS)
        assert (lc.expected("rgb", w, h, win, 0, "invalid").gray[bad] == 0).all()


# ---- the same cases on the unfused kernels --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unfused_lines():
    env = dict(os.environ)
    env["POLYCHASE_PYRAMID_VARIANT"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_lens_check.py")], env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, f"the helper failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", lc.case_names())
def test_unfused_kernels_match_the_rule(unfused_lines, name):
    mine = [l for l in unfused_lines if l.split()[1:2] == [name]]
    assert mine == [f"PASS {name}"], mine


# ---- the other promises of the header -------------------------------------------------------------------------------
W, H, WIN = 131, 34, 10


def _planes(frame):
    out = [frame.gray()]
    for l in range(frame.num_levels):
        out += [frame.level(l), frame.deriv(l), frame.level16(l)]
    return [a.tobytes() for a in out]


def _put(c, frame, kind, which=0):
    img = check.image(kind, frame.w, frame.h, which)
    keep, rc = check.put(c, frame, kind, img, 0, check.row_bytes_of(kind, frame.w), "pageable", seed=7)
    assert rc == 0, hip.load().pc_last_error().decode()
    planes = _planes(frame)
    keep.release()
    return planes


def _timed_put(c, kind):
    """(planes, launches per timing class) of one frame put on context c"""
    frame = hip.Frame(c, W, H, WIN, 3)
    c.synchronize()
    c.enable_timing(True)
    c.reset_timing()
    try:
        planes = _put(c, frame, kind)
        counts = {k: v[0] for k, v in c.timing().items()}
    finally:
        c.enable_timing(False)
        frame.close()
    return planes, counts


@pytest.mark.parametrize("kind", check.KINDS)
def test_identity_and_cleared_maps_against_a_context_that_never_set_one(kind):
    plain, used = hip.Context(0), hip.Context(0)
    try:
        assert plain.lens_map_size() == (0, 0) and used.lens_map_size() == (0, 0)
        want_planes, want_counts = _timed_put(plain, kind)
        live = hip.live_resources()[0]
        used.set_lens_map(ref.identity_map(W, H))
        assert used.lens_map_size() == (W, H)
        assert hip.live_resources()[0] == live + 3, "the map and the two planes"
        got_planes, got_counts = _timed_put(used, kind)
        assert got_planes == want_planes, "with q = 256 (u, v) the remap is the gray plane itself, bit for bit"
        print("launches without a map", want_counts, "with one", got_counts)
        assert got_counts["gray"] == want_counts["gray"] + 2, "the gray kernel and the remap, both counted under PC_K_GRAY"
        assert {k: v for k, v in got_counts.items() if k != "gray"} == {k: v for k, v in want_counts.items() if k != "gray"}
        live = hip.live_resources()[0]
        used.set_lens_map(None)
        assert used.lens_map_size() == (0, 0) and hip.live_resources()[0] == live - 3
        used.set_lens_map(None)                                            # clearing nothing is fine
        got_planes, got_counts = _timed_put(used, kind)
        assert got_planes == want_planes and got_counts == want_counts, "a cleared map leaves no trace"
    finally:
        plain.close()
        used.close()


def test_a_frame_of_another_size_is_refused_and_keeps_its_planes(ctx):
    L = hip.load()
    small = hip.Frame(ctx, 65, 17, WIN, 3)
    try:
        before = _put(ctx, small, "rgb", 0)
        ctx.set_lens_map(lc.lens_map("pincushion", W, H))
        for kind in check.KINDS:
            img = check.image(kind, 65, 17, 1)
            for where in il.PLACEMENTS:
                keep, rc = check.put(ctx, small, kind, img, 0, check.row_bytes_of(kind, 65), where, seed=9)
                ctx.synchronize()
                keep.release()
                assert rc == PC_E_INVALID and "lens map" in L.pc_last_error().decode(), (kind, where)
        assert _planes(small) == before
        # a refused setter changes nothing: the map in force stays, bit for bit
        q = lc.lens_map("random", W, H)
        for w, h in ((0, H), (W, 0), (-1, H), (1 << 16, (1 << 14) + 1)):
            assert L.pc_context_set_lens_map(ctx._h, q.ctypes.data, w, h) == PC_E_INVALID
        assert L.pc_context_set_lens_map(None, q.ctypes.data, W, H) == PC_E_INVALID
        with pytest.raises(ValueError):
            ctx.set_lens_map(q.astype(np.int64))
        assert ctx.lens_map_size() == (W, H)
        frame = hip.Frame(ctx, W, H, WIN, 3)
        try:
            assert lc._put_and_compare(ctx, frame, "rgb", "device", 0, lc._pitch("rgb", W, None), 0, 11,
                                       lc.expected("rgb", W, H, WIN, 0, "pincushion")) == ""
            # a new map replaces the one in force
            ctx.set_lens_map(q)
            assert lc._put_and_compare(ctx, frame, "rgb", "device", 0, lc._pitch("rgb", W, None), 0, 11,
                                       lc.expected("rgb", W, H, WIN, 0, "random")) == ""
        finally:
            frame.close()
        ctx.set_lens_map(None)
        assert _put(ctx, small, "rgb", 0) == before, "and without a map the small frame is taken again"
    finally:
        ctx.set_lens_map(None)
        small.close()


def test_detection_and_lk_see_the_undistorted_frames(ctx):
    """the recipe scene (tests/test_lens_cpu.py) cropped to 131 x 98: the crop's offset moves the model's principal point"""
    w, h, win, ox, oy = 131, 98, 10, 94, 71
    m = dict(ref.recipe_model(320, 240), cx=159.5 - ox, cy=119.5 - oy)
    _, dist = ref.scene_frames(w, h, m, [(0.0, 0.0), (5.3, -3.6), (-2.2, 1.4)], seed=1)
    q = hip.lens_build_map(hip.lens_model(**m), w, h)
    assert np.array_equal(q, ref.build_map(m, w, h))
    und = [ref.remap(g, q) for g in dist]
    assert not np.array_equal(und[0], dist[0])
    ctx.set_lens_map(q)
    frames = [hip.Frame(ctx, w, h, win, 3) for _ in dist]
    try:
        for f, g in zip(frames, dist):
            f.set_gray(g)
        frames[0].detect()
        kps = frames[0].keypoints()
        okps = oracle.gftt(und[0])
        assert len(kps) > 50 and np.array_equal(kps, okps)
        assert not np.array_equal(okps, oracle.gftt(dist[0])), "the distorted frame has other corners"
        opt = hip.flow_options(window_size=win, max_level=3)
        xy, st, err = hip.lk_track(ctx, frames[0], frames[1:], opt)
        oopt = oracle.flow_options(window_size=win, max_level=3)
        p0 = oracle.Pyramid(und[0], win, 3)
        for k in (0, 1):
            oxy, ost, oerr = oracle.lk(p0, oracle.Pyramid(und[k + 1], win, 3), kps, oopt)
            assert np.array_equal(st[k], ost) and ost.sum() > 40
            ok = ost == 1
            assert np.array_equal(xy[k][ok].view(np.uint32), oxy[ok].view(np.uint32))
            assert np.array_equal(err[k][ok].view(np.uint32), oerr[ok].view(np.uint32))
    finally:
        for f in frames:
            f.close()
        ctx.set_lens_map(None)
