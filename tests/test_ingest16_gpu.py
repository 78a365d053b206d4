"""GPU: uint16, float16 and RGBA frames at the C ABI (pc_frame_set_pixels), converted on the GPU -- against the numpy restatement
of the channel rules (tests/ingest16_ref.py) fed to the CPU oracle.  Everything is bit-exact; nothing is a tolerance.

  * exhaustive: a 256 x 256 frame per 16-bit type holds every value / pattern in each channel; the gray plane under the default
    conversion, under weights that show one channel's bytes and, for halves, under a transfer table whose entries tell the
    subnormals apart;
  * layouts: tests/_ingest16_check.py has the case list (sizes at the tile edges x kinds x placements x base offsets x pitch gaps);
  * a reused frame, refused calls (PC_E_INVALID by argument checks, planes intact), the old entry points' types through the new
    call, the unfused kernels in a child process under POLYCHASE_PYRAMID_VARIANT=1, and the lens path."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ingest16_check as check
import _ingest_check as base
import gray_conversion_ref as gref
import ingest16_ref as ref
import ingest_layouts as il
from polychase_amd import hip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALL16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


# ---- every value of a 16-bit channel --------------------------------------------------------------------------------
def _every_pattern(dtype, channels):
    """R holds the pattern, G the pattern reversed, B a fixed permutation; alpha is noise"""
    rng = np.random.default_rng(77)
    planes = [ALL16, ALL16[::-1], rng.permutation(ALL16)]
    if channels == 4:
        planes.append(rng.integers(0, 65536, 65536).astype(np.uint16))
    img = np.ascontiguousarray(np.stack(planes, axis=1).reshape(256, 256, channels)).view(dtype)
    img.setflags(write=False)
    return img


CONVERSIONS = [("default", None, None), ("blue", (0, 0, 32768), None), ("red", (32768, 0, 0), None), ("green", (0, 32768, 0), None),
               ("srgb_exposure_14", None, ("srgb", 14.0))]


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("dtype", [np.uint16, np.float16], ids=["uint16", "float16"])
def test_every_value_of_a_16_bit_channel(ctx, dtype, channels):
    img = _every_pattern(dtype, channels)
    frame = hip.Frame(ctx, 256, 256, 5, 0)
    try:
        for name, weights, curve in CONVERSIONS:
            if curve and dtype != np.float16:
                continue                      # a transfer table does nothing for integer frames
            table = gref.table(curve[0], exposure=curve[1]) if curve else None
            ctx.set_gray_conversion(weights, table)
            frame.set_pixels(img)
            got = frame.gray()
            want = ref.gray_expected(img, weights, table)
            assert np.array_equal(got, want), (name, int(np.count_nonzero(got != want)))
            if weights and max(weights) == 32768:      # ... which is that channel's bytes exactly
                assert np.array_equal(got, ref.channel_bytes(img, table)[:, :, int(np.argmax(weights))])
        if dtype == np.float16:
            # the table's entries tell the subnormal halves between 2^-16 and 2^-14 apart: a flushed one would show
            tab = gref.table("srgb", exposure=14.0)
            sub = ALL16[(ALL16 >= 0x0100) & (ALL16 < 0x0400)]
            assert len(np.unique(tab[gref.transfer_index(ref.f16_bits_to_f32(sub))])) > 100
    finally:
        ctx.set_gray_conversion()
        frame.close()


# ---- the layouts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", check.layout_cases(), ids=check.layout_name)
def test_planes_of_every_layout_match_the_oracle(ctx, case):
    assert os.environ.get("POLYCHASE_PYRAMID_VARIANT", "0") == "0", "this process must run the fused level kernel"
    assert check.run_layout_case(ctx, case) == ""


def test_the_case_list_covers_what_it_claims():
    assert {(w, h) for w, h, _ in check.SIZES} == {(63, 15), (64, 16), (65, 17), (66, 33), (67, 35), (129, 18), (23, 19)}
    assert {w % 4 for w, _, _ in check.SIZES} == {0, 1, 2, 3}
    assert len(check.layout_cases()) == 5 * 4 * 7
    for kind in check.KINDS:
        for w, _, _ in check.SIZES:
            rb = check.row_bytes_of(kind, w)
            lay = check.layouts_of(kind, w)
            assert {p - rb for _, p in lay} == {0, 2, 6, check.BIG_GAP} and check.BIG_GAP > rb
            assert {o % 4 for o, _ in lay} == ({0, 1, 2, 3} if kind == "rgba8" else {0, 2})
        # both the dword path (pointer and pitch multiples of 4) and the per-pixel path occur for every kind
        al = {(o | p) % 4 == 0 for w, _, _ in check.SIZES for o, p in check.layouts_of(kind, w)}
        assert al == {True, False}, kind
        for w, h, win in check.SIZES:
            a, b = check.expected(kind, w, h, win, 0), check.expected(kind, w, h, win, 1)
            assert not np.array_equal(a.gray, b.gray) and not np.array_equal(a.level16[-1], b.level16[-1])
    for which in (0, 1):
        img = check.image("rgbaf16", 63, 15, which)
        assert set(check._f16_extremes().view(np.uint16).tolist()) <= set(img[:, :, :3].view(np.uint16).ravel().tolist())
        assert np.isnan(img[:, :, 3]).all()
        img = check.image("rgb16", 63, 15, which)
        assert set(check._u16_extremes().tolist()) <= set(img.ravel().tolist())


# ---- reuse ----------------------------------------------------------------------------------------------------------
def test_a_frame_that_held_a_uint8_image_holds_the_float16_image_put_next(ctx):
    w, h, win = 67, 35, 5
    frame = hip.Frame(ctx, w, h, win, check.MAX_LEVEL)
    try:
        frame.set_rgb(np.array(base.image("rgb", w, h, 0)))
        assert base.planes_mismatch(frame, base.expected("rgb", w, h, win, 0)) == ""
        frame.set_pixels(np.array(check.image("rgbf16", w, h, 1)))
        assert base.planes_mismatch(frame, check.expected("rgbf16", w, h, win, 1)) == ""
    finally:
        frame.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rgb16", "rgbaf16"])
def test_refused_calls_leave_the_planes_intact(ctx, kind):
    w, h, win = 67, 35, 5
    frame = hip.Frame(ctx, w, h, win, check.MAX_LEVEL)
    keep, rc = check.put(ctx, frame, check.image(kind, w, h, 0), 0, check.row_bytes_of(kind, w), "pageable", seed=1)
    assert rc == 0
    e = check.expected(kind, w, h, win, 0)
    assert base.planes_mismatch(frame, e) == ""
    rb, ch, ptype = check.row_bytes_of(kind, w), check.CHANNELS[kind], ref.PIXEL_TYPE[np.dtype(check.DTYPE[kind])]
    # pageable host memory with room for the widest call below (5 channels of 4 bytes, a full pitch): a call that is NOT refused
    # reads nothing outside
    buf = np.random.default_rng(9).integers(0, 256, 16 + h * w * 5 * 4, dtype=np.uint8)
    assert buf.ctypes.data % 4 == 0
    calls = [("odd pointer", 1, rb, ptype, ch), ("odd pitch", 0, rb + 1, ptype, ch), ("pitch below a row", 0, rb - 2, ptype, ch),
             ("1 channel", 0, w * 2, ptype, 1), ("2 channels", 0, w * 4, ptype, 2), ("5 channels", 0, w * 10, ptype, 5),
             ("pixel type 4", 0, rb, 4, ch), ("pixel type -1", 0, rb, -1, ch), ("2 channels of uint8", 0, w * 2, ref.PIXEL_U8, 2)]
    for what, off, pitch, pt, channels in calls:
        rc = check.set_pixels(ctx, frame, buf.ctypes.data + off, pitch, pt, channels, 0)
        assert rc == base.PC_E_INVALID, (what, rc)
        assert base.planes_mismatch(frame, e) == "", what
    keep.release()
    frame.close()


# ---- the types of the old entry points through the new one -----------------------------------------------------------
def _planes(frame):
    out = [frame.gray()]
    for l in range(frame.num_levels):
        out += [frame.level(l), frame.deriv(l), frame.level16(l)]
    return out


@pytest.mark.parametrize("kind", ["rgb", "gray", "f32x4"])
def test_old_pixel_types_through_the_new_call_give_the_old_calls_planes(ctx, kind):
    w, h, win = 67, 35, 5
    img = np.array(base.image(kind, w, h, 0))
    old, new = hip.Frame(ctx, w, h, win, base.MAX_LEVEL), hip.Frame(ctx, w, h, win, base.MAX_LEVEL)
    try:
        (old.set_gray if kind == "gray" else old.set_rgb)(img)
        new.set_pixels(img)
        assert base.planes_mismatch(old, base.expected(kind, w, h, win, 0)) == ""
        a, b = _planes(old), _planes(new)
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    finally:
        old.close()
        new.close()


# ---- the unfused kernels --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unfused_lines():
    env = dict(os.environ)
    env["POLYCHASE_PYRAMID_VARIANT"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_ingest16_check.py")], env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, f"the helper failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", check.unfused_names())
def test_unfused_kernels_match_the_oracle(unfused_lines, name):
    mine = [l for l in unfused_lines if l.split()[1:2] == [name]]
    assert mine == [f"PASS {name}"], mine


def test_the_unfused_list_has_an_aligned_and_a_misaligned_layout_per_kind():
    for kind in check.KINDS:
        lay = check.unfused_layouts(kind)
        rb = check.row_bytes_of(kind, check.UNFUSED_SIZE[0])
        assert [(o | p) % 4 == 0 for o, p in lay] == [True, False] and all(p >= rb for _, p in lay)


# ---- the lens path --------------------------------------------------------------------------------------------------
def test_under_a_lens_map_the_16_bit_frames_give_their_8_bit_and_float32_frames_planes(ctx):
    w, h, win = 131, 67, 5
    model = hip.lens_model(fx=120.0, fy=120.0, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, k1=-0.15)
    ctx.set_lens_map(hip.lens_build_map(model, w, h))
    frames = [hip.Frame(ctx, w, h, win, base.MAX_LEVEL) for _ in range(2)]
    try:
        rng = np.random.default_rng(3)
        u8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        frames[0].set_rgb(u8)
        frames[1].set_pixels(u8.astype(np.uint16) * np.uint16(257))
        a, b = _planes(frames[0]), _planes(frames[1])
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), "uint16 (x * 257) under the lens map"
        assert not np.array_equal(a[0], il.gray_of(u8)), "the map must move pixels"
        half = rng.integers(0, 0x3c01, (h, w, 4)).astype(np.uint16).view(np.float16)
        frames[0].set_rgb(half.astype(np.float32))
        frames[1].set_pixels(half)
        a, b = _planes(frames[0]), _planes(frames[1])
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), "float16 under the lens map"
    finally:
        ctx.set_lens_map(None)
        for f in frames:
            f.close()
