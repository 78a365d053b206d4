"""CPU: lens undistortion at ingest (include/polychase_hip.h: pc_lens_model, pc_context_set_lens_map).  The host-side makers of a
lens map -- pc_lens_build_map, pc_lens_map_from_stmap, pc_lens_map_valid -- against the numpy restatement of the rule
(tests/lens_ref.py), every int32 and every byte equal; their refusals; the remap kernel's register and LDS budget read from the
built library; and that the rule does its job, shown on the CPU oracle alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import lens_ref as ref
import oracle
import test_kernel_resources_cpu as resources
from polychase_amd import build, hip

PC_E_INVALID = -1
SIZES = [(37, 29), (320, 240)]


def _centre(w, h):
    return (w - 1) / 2.0, (h - 1) / 2.0


def _models(w, h):
    cx, cy = _centre(w, h)
    f = 0.9375 * w
    return {
        "zero": ref.model(f, f, cx, cy),
        "barrel": ref.model(f, f, cx, cy, k1=-0.15, k2=0.02, p1=0.001, p2=-0.0005),
        "pincushion": ref.pincushion(w, h),
        "tangential": ref.model(f, 1.1 * f, cx + 0.25, cy - 1.5, p1=0.02, p2=-0.03),
        "zoom_0.85": ref.model(f, f, cx, cy, k1=-0.15, k2=0.02, zoom=0.85),
        "zoom_1.2": ref.model(f, f, cx, cy, k1=0.1, k3=0.01, zoom=1.2),
        # a focal length of a hundredth of a pixel: x reaches 1e4, r2^3 k3 1e24 -- beyond the clamp everywhere but the centre
        "beyond_clamp": ref.model(0.01, 0.01, cx, cy, k1=1.0, k2=1.0, k3=1.0),
        # ... and coefficients whose products overflow fp64: inf - inf at the corners
        "non_finite": ref.model(0.01, 0.01, cx, cy, k1=1e300, k2=-1e300, k3=1e300, p1=1e300, p2=-1e300),
    }


def _abi_model(m):
    return hip.lens_model(**m)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_build_map_equals_the_restatement(size):
    w, h = size
    for name, m in _models(w, h).items():
        got = hip.lens_build_map(_abi_model(m), w, h)
        want = ref.build_map(m, w, h)
        assert got.dtype == np.int32 and got.shape == (h, w, 2)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:3])
        if name == "zero":
            assert np.array_equal(got, ref.identity_map(w, h)), "all-zero coefficients: q == 256 (u, v) exactly"
        if name == "beyond_clamp":
            assert (np.abs(got) == ref.CLAMP).any() and not (got == ref.INVALID).any()
        if name == "non_finite":
            bad = got[..., 0] == ref.INVALID
            assert bad.any() and np.array_equal(bad, got[..., 1] == ref.INVALID), "a non-finite position invalidates both components"
        if name in ("barrel", "pincushion", "tangential"):
            assert not np.array_equal(got, ref.identity_map(w, h)) and np.abs(got).max() < ref.CLAMP


def test_default_model():
    m = hip.LensModel()
    hip.load().pc_lens_default_model(C.byref(m))
    assert [getattr(m, k) for k in ref.FIELDS] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("flip_v", [True, False])
def test_stmap_conversion(flip_v):
    w, h = 37, 29
    rng = np.random.default_rng(5)
    st = rng.uniform(-0.2, 1.2, (h, w, 2)).astype(np.float32)              # also outside [0, 1]
    # an STmap that means "identity": pixel centre i at (i + 0.5) / w
    ident = np.stack(np.broadcast_arrays((np.arange(w)[None, :] + 0.5) / w, (np.arange(h)[:, None] + 0.5) / h), axis=2).astype(np.float32)
    if flip_v:
        ident[..., 1] = 1.0 - ident[..., 1]
    st[0, 0] = (np.nan, 0.5)
    st[1, 2] = (0.5, np.nan)
    st[2, 3] = (np.inf, 0.25)
    st[3, 4] = (0.25, -np.inf)
    st[4, 5] = (3e38, -3e38)                                               # finite, far beyond the clamp
    got = hip.lens_map_from_stmap(st, flip_v)
    assert np.array_equal(got, ref.map_from_stmap(st, flip_v))
    for y, x in ((0, 0), (1, 2), (2, 3), (3, 4)):
        assert tuple(got[y, x]) == (ref.INVALID, ref.INVALID)
    assert (tuple(got[4, 5]) == (ref.CLAMP, ref.CLAMP)) if flip_v else (tuple(got[4, 5]) == (ref.CLAMP, -ref.CLAMP))
    qi = hip.lens_map_from_stmap(ident, flip_v)
    assert np.array_equal(qi, ref.map_from_stmap(ident, flip_v))
    assert np.abs(qi - ref.identity_map(w, h)).max() <= 1, "the centres of an identity STmap, up to float32 rounding of s and t"


@functools.lru_cache(maxsize=None)
def _pincushion_map(w=320, h=240):
    q = hip.lens_build_map(_abi_model(ref.pincushion(w, h)), w, h)
    q.setflags(write=False)
    return q


@pytest.mark.parametrize("erode", [0, 1, 6, 11])
def test_validity_and_erosion(erode):
    q = _pincushion_map()
    got = hip.lens_map_valid(q, erode)
    want = ref.valid(q, erode)
    assert got.dtype == np.uint8 and set(np.unique(got)) == {0, 255}
    assert np.array_equal(got, want)
    off = float((got == 0).mean())
    print("pincushion 320x240, erode %d: %.1f %% of the pixels are off" % (erode, 100 * off))
    assert 0.01 <= off <= 0.60
    all_valid = C.c_int(-1)
    assert hip.load().pc_lens_map_valid(q.ctypes.data, 320, 240, erode, got.ctypes.data, C.byref(all_valid)) == 0 and all_valid.value == 0


def test_validity_of_small_and_all_valid_maps():
    w, h = 37, 29
    ident = ref.identity_map(w, h)
    for erode in (0, 3, 64):
        out = np.zeros((h, w), np.uint8)
        all_valid = C.c_int(-1)
        assert hip.load().pc_lens_map_valid(ident.ctypes.data, w, h, erode, out.ctypes.data, C.byref(all_valid)) == 0
        assert all_valid.value == 1 and (out == 255).all(), "an erosion judges only pixels inside the frame"
    rng = np.random.default_rng(3)
    q = rng.integers(-2 * 256, (w + 1) * 256, (h, w, 2)).astype(np.int32)
    q[..., 1] = rng.integers(-2 * 256, (h + 1) * 256, (h, w))
    q[5, 7] = ref.INVALID
    q[6, 8] = ((w - 1) * 256, (h - 1) * 256)                              # the last valid position
    q[6, 9] = ((w - 1) * 256 + 1, 0)                                       # one step beyond
    for erode in (0, 1, 2, 40):
        assert np.array_equal(hip.lens_map_valid(q, erode), ref.valid(q, erode)), erode
    assert hip.lens_map_valid(q, 0)[6, 8] == 255 and hip.lens_map_valid(q, 0)[6, 9] == 0


def test_refusals_leave_the_output_untouched():
    L = hip.load()
    w, h = 8, 6
    sentinel = np.full((h, w, 2), 12345, np.int32)
    good = ref.model(10.0, 10.0, 3.5, 2.5)

    def build(m, ww=w, hh=h):
        q = sentinel.copy()
        rc = L.pc_lens_build_map(C.byref(_abi_model(m)), ww, hh, q.ctypes.data)
        assert np.array_equal(q, sentinel) or rc == 0
        return rc

    assert build(good) == 0
    for field in ref.FIELDS:
        for bad in (np.nan, np.inf, -np.inf):
            assert build(dict(good, **{field: bad})) == PC_E_INVALID, (field, bad)
    for field in ("fx", "fy", "zoom"):
        for bad in (0.0, -1.0):
            assert build(dict(good, **{field: bad})) == PC_E_INVALID, (field, bad)
    # sizes pc_frame_create refuses: below 1, more than 2^30 pixels (refused before a single entry is written)
    for ww, hh in ((0, h), (w, 0), (-3, h), (1 << 16, (1 << 14) + 1)):
        assert build(good, ww, hh) == PC_E_INVALID, (ww, hh)
        st = np.zeros((h, w, 2), np.float32)
        q = sentinel.copy()
        assert L.pc_lens_map_from_stmap(st.ctypes.data, ww, hh, 1, q.ctypes.data) == PC_E_INVALID and np.array_equal(q, sentinel)
        out = np.full((h, w), 77, np.uint8)
        av = C.c_int(-7)
        assert L.pc_lens_map_valid(sentinel.ctypes.data, ww, hh, 0, out.ctypes.data, C.byref(av)) == PC_E_INVALID
        assert (out == 77).all() and av.value == -7
    for erode in (-1, 65, 1000):
        out = np.full((h, w), 77, np.uint8)
        av = C.c_int(-7)
        assert L.pc_lens_map_valid(sentinel.ctypes.data, w, h, erode, out.ctypes.data, C.byref(av)) == PC_E_INVALID, erode
        assert (out == 77).all() and av.value == -7 and "erode" in L.pc_last_error().decode()
    # null arguments
    assert L.pc_lens_build_map(None, w, h, sentinel.ctypes.data) == PC_E_INVALID
    assert L.pc_lens_build_map(C.byref(_abi_model(good)), w, h, None) == PC_E_INVALID
    assert L.pc_lens_map_from_stmap(None, w, h, 1, sentinel.ctypes.data) == PC_E_INVALID
    assert L.pc_lens_map_valid(None, w, h, 0, sentinel.ctypes.data, None) == PC_E_INVALID
    # the setters refuse a null context before anything else
    assert L.pc_context_set_lens_map(None, sentinel.ctypes.data, w, h) == PC_E_INVALID
    assert L.pc_context_get_lens_map_size(None, None, None) == PC_E_INVALID
    # the Python surface says ValueError
    with pytest.raises(ValueError):
        hip.lens_build_map(_abi_model(dict(good, fx=0.0)), w, h)
    with pytest.raises(ValueError):
        hip.lens_map_valid(sentinel, 65)
    with pytest.raises(ValueError):
        hip.lens_map_valid(sentinel.astype(np.int64), 0)
    with pytest.raises(ValueError):
        hip.lens_map_from_stmap(np.zeros((h, w, 2), np.float64))


def test_symbols_and_binding():
    L = hip.load()
    for s in ("pc_lens_default_model", "pc_lens_build_map", "pc_lens_map_from_stmap", "pc_lens_map_valid", "pc_context_set_lens_map",
              "pc_context_get_lens_map_size"):
        assert s in hip.SYMBOLS and hasattr(L, s), s
    assert callable(hip.Context.set_lens_map) and callable(hip.Context.lens_map_size)
    assert hip.LENS_FRAC_BITS == ref.FRAC_BITS == 8 and hip.LENS_INVALID == ref.INVALID == -2 ** 31


def test_remap_kernel_fits_beside_three_lk_wavefronts():
    """at most 104 VGPRs allocated and no LDS, like the other helpers (tests/test_kernel_resources_cpu.py reads the same notes)"""
    path = build.hip_library_path()
    kernels = {k[".name"]: k for elf in resources._code_objects(path) for k in resources._kernel_metadata(elf)}
    found = [k for n, k in kernels.items() if "lens_remap_kernel" in n]
    assert len(found) == 1
    k = found[0]
    print("lens_remap_kernel: %d VGPRs, %d B of LDS" % (k[".vgpr_count"], k[".group_segment_fixed_size"]))
    assert (k[".vgpr_count"] + 7) // 8 * 8 <= resources.HELPER_VGPR_BUDGET == 104
    assert k[".group_segment_fixed_size"] == 0
    assert k.get(".agpr_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0


# ---- the rule does its job: the CPU oracle alone ----------------------------------------------------------------------
W, H, SHIFT, SEED = 320, 240, (5.3, -3.6), 1


@functools.lru_cache(maxsize=None)
def _scene():
    m = ref.recipe_model(W, H)
    assert (m["cx"], m["cy"], m["fx"]) == (159.5, 119.5, 300.0)
    pin, dist = ref.scene_frames(W, H, m, [(0.0, 0.0), SHIFT], seed=SEED)
    q = ref.build_map(m, W, H)
    return pin, dist, [ref.remap(f, q) for f in dist]


def _median_error(frames, win):
    """median end-point error of the oracle's LK rows (status 1) against the true flow of the undistorted scene"""
    kps = oracle.gftt(frames[0])
    border = win + 8
    keep = (kps[:, 0] >= border) & (kps[:, 0] <= W - 1 - border) & (kps[:, 1] >= border) & (kps[:, 1] <= H - 1 - border)
    kps = kps[keep]
    assert len(kps) > 200
    fopt = oracle.flow_options(window_size=win)
    p0, p1 = oracle.Pyramid(frames[0], win, fopt.max_level), oracle.Pyramid(frames[1], win, fopt.max_level)
    out, st, _ = oracle.lk(p0, p1, kps, fopt)
    ok = st == 1
    assert ok.mean() > 0.9
    d = out[ok].astype(np.float64) - kps[ok].astype(np.float64) - np.array(SHIFT)
    return float(np.median(np.hypot(d[:, 0], d[:, 1])))


@pytest.mark.parametrize("win", [10, 21])
def test_the_remap_recovers_the_pinhole_floor(win):
    """320 x 240, f = 300, k1 = -0.15, k2 = 0.02, p1 = 0.001, p2 = -0.0005, a pan of (5.3, -3.6), texture seed 1.  Median
    end-point error of the oracle's LK rows, measured with this file's seed:
        window 10: pinhole 0.0268 px, distorted as they are 0.2445 px (9.1 x), after lens_ref.remap 0.0278 px (1.04 x)
        window 21: pinhole 0.0200 px, distorted as they are 0.1612 px (8.1 x), after lens_ref.remap 0.0192 px (0.96 x)
    The bounds are the issue's: <= 1.25 x the pinhole median after the remap, >= 4 x on the distorted frames as they are."""
    pin, dist, undist = _scene()
    floor, raw, fixed = _median_error(pin, win), _median_error(dist, win), _median_error(undist, win)
    print("window %d: pinhole %.4f px, distorted %.4f px (%.1f x), remapped %.4f px (%.2f x)" % (win, floor, raw, raw / floor, fixed, fixed / floor))
    assert fixed <= 1.25 * floor
    assert raw >= 4.0 * floor
