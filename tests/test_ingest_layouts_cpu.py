"""CPU: the helpers of tests/ingest_layouts.py that the frame-ingestion GPU tests stand on -- the buffer lay_out builds, the
float -> u8 rule and the expected planes."""
import numpy as np
import pytest

import ingest_layouts as il

# the values the issue's check of the rule against numpy's cast was made on
LISTED = [np.nan, np.inf, -np.inf, 1e10, -1e10, 8421504.3, -8421504.3, 1.5, -0.1, 2.0, 1.0, 0.999999, 2147483520 / 255]


def _images():
    rng = np.random.default_rng(11)
    return [rng.integers(0, 256, (7, 13, 3), dtype=np.uint8), rng.integers(0, 256, (5, 9), dtype=np.uint8),
            rng.uniform(-1, 2, (6, 11, 3)).astype(np.float32), rng.uniform(-1, 2, (4, 10, 4)).astype(np.float32)]


@pytest.mark.parametrize("k", range(4))
def test_pageable_layout_round_trips_and_has_exactly_the_promised_length(k):
    img = _images()[k]
    unit = 4 if img.dtype == np.float32 else 1
    rb = il.row_bytes(img)
    assert rb == img[0].nbytes
    for offset, gap in ((0, 0), (unit, 0), (3 * unit, 13 * unit), (2 * unit, rb + 4100)):
        pitch = rb + gap
        keep, address, got_pitch, on_device = il.lay_out(img, offset, pitch, "pageable", seed=5)
        assert (got_pitch, on_device) == (pitch, 0)
        assert address == keep.buffer.ctypes.data + offset
        assert keep.buffer.dtype == np.uint8 and keep.buffer.ndim == 1
        assert len(keep.buffer) == offset + pitch * (img.shape[0] - 1) + rb == il.buffer_size(img, offset, pitch)
        back = il.pixels_of(keep.buffer, img, offset, pitch)
        assert back.dtype == img.dtype and np.array_equal(back.view(np.uint8), img.view(np.uint8))
        keep.release()


def test_two_seeds_give_different_poison_and_the_same_pixels():
    img = _images()[0]
    rb, offset, pitch = il.row_bytes(img), 3, il.row_bytes(img) + 13
    a, b = il.fill(img, offset, pitch, 1), il.fill(img, offset, pitch, 2)
    assert np.array_equal(il.pixels_of(a, img, offset, pitch), img) and np.array_equal(il.pixels_of(b, img, offset, pitch), img)
    is_pixel = np.zeros(len(a), bool)
    for y in range(img.shape[0]):
        is_pixel[offset + y * pitch: offset + y * pitch + rb] = True
    assert np.array_equal(a[is_pixel], b[is_pixel])
    poison_a, poison_b = a[~is_pixel], b[~is_pixel]
    assert len(poison_a) == offset + 13 * (img.shape[0] - 1)
    assert (poison_a != poison_b).mean() > 0.9
    assert len(np.unique(poison_a)) > 16          # noise, not a constant
    assert np.array_equal(il.fill(img, offset, pitch, 1), a)   # and seeded


def test_float_layouts_must_be_four_byte_aligned():
    img = _images()[2]
    with pytest.raises(AssertionError):
        il.fill(img, 2, il.row_bytes(img), 0)
    with pytest.raises(AssertionError):
        il.fill(img, 0, il.row_bytes(img) + 2, 0)


def test_float_to_u8_is_numpys_cast_on_finite_values_within_int32():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-2, 3, 3000), rng.uniform(-8421504, 8421504, 3000), rng.uniform(-300, 300, 500) / 255,
                        np.arange(-600, 600) / 255.0]).astype(np.float32)
    listed = np.array([v for v in LISTED if np.isfinite(v) and abs(np.float32(v) * np.float32(255)) < 2.0 ** 31], np.float32)
    assert len(listed) == 8
    x = np.concatenate([x, listed])
    s = x * np.float32(255)
    assert np.isfinite(s).all() and (np.abs(s) < 2.0 ** 31).all()
    assert np.array_equal(il.float_to_u8(x), s.astype(np.int32).astype(np.uint8))   # defined: in range of int32, then modulo 2^8
    with np.errstate(invalid="ignore"):
        assert np.array_equal(il.float_to_u8(x), (x * 255).astype(np.uint8))        # the addon's expression, a recorded fact here
    assert il.float_to_u8(x).shape == x.shape and il.float_to_u8(x).dtype == np.uint8


def test_float_to_u8_known_values():
    up = np.nextafter(np.float32(2.0 ** 31 / 255), np.float32(np.inf))   # 2^31 / 255 rounded up: the product is 2^31
    assert np.float32(up) * np.float32(255) >= np.float32(2.0 ** 31)
    zeros = np.array([np.nan, np.inf, -np.inf, 1e10, -1e10, up], np.float32)
    assert np.array_equal(il.float_to_u8(zeros), np.zeros(6, np.uint8))
    below = np.float32(8421504.3)                                        # the product is 2^31 - 128: the last one in range
    assert float(below) * 255 == 2.0 ** 31 - 128
    x = np.array([below, -below, 1.5, -0.1, 2.0, 1.0, 0.999999, 0.0, -0.0, 1e-40, 1 / 255, 254.999 / 255], np.float32)
    want = [(2 ** 31 - 128) & 0xff, (-(2 ** 31 - 128)) & 0xff, 382 & 0xff, (-25) & 0xff, 510 & 0xff, 255, 254, 0, 0, 0, 1, 254]
    assert il.float_to_u8(x).tolist() == want
    assert il.float_to_u8(np.float32(-2.0 ** 31 / 255 * 1.0000001)).tolist() == 0   # below -2^31: out of range too


def test_expected_planes():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (35, 67, 3), dtype=np.uint8)
    e = il.expected(rgb, 5, 3)
    assert e.num_levels == 3 and e.sizes == [(67, 35), (34, 18), (17, 9)]
    assert e.gray.shape == (35, 67) and np.array_equal(e.level[0][5:-5, 5:-5], e.gray)
    for l in range(e.num_levels):
        w, h = e.sizes[l]
        assert e.level[l].shape == e.level16[l].shape == (h + 10, w + 10) and e.deriv[l].shape == (h + 10, w + 10, 2)
        assert e.level16[l].dtype == np.uint16 and e.deriv[l].dtype == np.int16
        assert np.array_equal(e.level16[l], e.level[l].astype(np.uint16) << 7)      # the whole padded plane
        assert int(e.level16[l].max()) == int(e.level[l].max()) * 128 <= 255 * 128
        assert not e.level16[l].flags.writeable
    # the padding is REFLECT_101 and a window wider than the image reflects more than once
    assert np.array_equal(e.level[0][5:-5, 0], e.gray[:, 5]) and np.array_equal(e.level[0][0, 5:-5], e.gray[5, :])
    small = il.expected(rgb[:19, :23], 25, 3)
    assert small.num_levels == 1 and small.level[0].shape == (69, 73)
    # gray input is taken as it is; float input goes through float_to_u8 with alpha dropped
    g = il.expected(e.gray, 5, 3)
    assert np.array_equal(g.gray, e.gray) and all(np.array_equal(a, b) for a, b in zip(g.level16, e.level16))
    f4 = np.concatenate([(rgb.astype(np.float32) + np.float32(0.5)) / np.float32(255), np.full((35, 67, 1), np.nan, np.float32)], axis=2)
    assert np.array_equal(il.float_to_u8(f4[:, :, :3]), rgb)
    f = il.expected(f4, 5, 3)
    assert np.array_equal(f.gray, e.gray) and all(np.array_equal(a, b) for a, b in zip(f.deriv, e.deriv))
