#!/usr/bin/env python3
"""Case list and runner of tests/test_ingest16_gpu.py: frames of the 16-bit and RGBA pixel types through pc_frame_set_pixels in
every source layout (base pointer, row_pitch, placement), against the numpy restatement of the channel rules
(tests/ingest16_ref.py) fed to the CPU oracle, bit for bit -- compared the way tests/_ingest_check.py compares (planes_mismatch:
gray; per level the padded u8 plane, the derivative plane and the uint16 plane; the level geometry).

A 16-bit image travels through ingest_layouts.lay_out as a 2-D byte view, so the poison in the pitch gap and in front of the
base is that helper's.  The test file runs the cases in its own process (the fused level kernel; 23 x 19 under a 25-px window
takes the unfused level-0 kernels there too) and, through main() below, a short list in a child process under
POLYCHASE_PYRAMID_VARIANT=1.  One line per case: "PASS <name>" or "FAIL <name> <what differs first>"."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _ingest_check as base  # noqa: E402
import ingest16_ref as ref  # noqa: E402
import ingest_layouts as il  # noqa: E402
from polychase_amd import hip  # noqa: E402

MAX_LEVEL = base.MAX_LEVEL
# both sides of the 64-column and the 16- and 32-row tile edges, two tiles and a column, every residue of w mod 4; 23 x 19 under a
# 25-px window does not fit the fused kernel at level 0
SIZES = [(63, 15, 5), (64, 16, 5), (65, 17, 5), (66, 33, 5), (67, 35, 5), (129, 18, 5), (23, 19, 25)]     # (w, h, window)
KINDS = ("rgba8", "rgb16", "rgba16", "rgbf16", "rgbaf16")
DTYPE = {"rgba8": np.uint8, "rgb16": np.uint16, "rgba16": np.uint16, "rgbf16": np.float16, "rgbaf16": np.float16}
CHANNELS = {"rgba8": 4, "rgb16": 3, "rgba16": 4, "rgbf16": 3, "rgbaf16": 4}
BIG_GAP = 1040                                   # a pitch gap larger than any row here (129 x 4 x 2 = 1032 bytes)
GAPS = (0, 2, 6, BIG_GAP)


def elem_of(kind):
    return np.dtype(DTYPE[kind]).itemsize


def row_bytes_of(kind, w):
    return w * CHANNELS[kind] * elem_of(kind)


def offsets_of(kind):
    return (0, 1, 2, 3) if kind == "rgba8" else (0, 2)


def layouts_of(kind, w):
    rb = row_bytes_of(kind, w)
    return [(o, rb + g) for g in GAPS for o in offsets_of(kind)]


# ---- contents -------------------------------------------------------------------------------------------------------
def _u16_extremes():
    # the ends, both sides of the first, a middle and the last rounding boundary (v = 257 k + 128 | 129), multiples of 257
    return np.array([0, 65535, 128, 129, 32767, 32768, 32896, 32897, 65406, 65407, 257, 256, 255, 65278, 1, 514], np.uint16)


def _f16_extremes():
    # 1, zeros, the largest below 1, above 1, negative, NaN, infinities, the largest half, subnormals (the smallest, the largest,
    # one between 2^-16 and 2^-15), the smallest normal, 1 / 255 and its neighbours' region
    bits = [0x3c00, 0x0000, 0x8000, 0x3bff, 0x3e00, 0xae66, 0x7e00, 0x7c00, 0xfc00, 0x7bff, 0x0001, 0x03ff, 0x0180, 0x0400, 0x1c04, 0xfe01]
    return np.array(bits, np.uint16).view(np.float16)


@functools.lru_cache(maxsize=None)
def image(kind, w, h, which):
    """image A (which = 0) or B (1) of a size: seeded noise, every extreme value in each channel along the middle row and at the
    special pixels of tests/_ingest_check.py; alpha is noise (NaN patterns for halves)"""
    rng = np.random.default_rng([w, h, which, 16 + KINDS.index(kind)])
    c, dt = CHANNELS[kind], DTYPE[kind]
    if dt == np.uint8:
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        ext = np.array([255, 0, 255, 0, 1, 254, 128, 127], np.uint8)
    elif dt == np.uint16:
        img = rng.integers(0, 65536, (h, w, c)).astype(np.uint16)
        ext = _u16_extremes()
    else:
        img = rng.integers(0, 0x3c01, (h, w, c)).astype(np.uint16).view(np.float16)     # every half of [0, 1], drawn as halves
        ext = _f16_extremes()
    for k, (x, y) in enumerate(base.special_pixels(w, h)):
        img[y, x, :3] = ext[(3 * k + 5 * which + np.arange(3)) % len(ext)]
    for k in range(len(ext)):
        img[h // 2, 1 + k, :3] = ext[(k + which + np.arange(3)) % len(ext)]
    if c == 4 and dt == np.float16:
        img[:, :, 3] = np.float16(np.nan)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(kind, w, h, win, which):
    return ref.planes_expected(image(kind, w, h, which), None, None, win, MAX_LEVEL)


def as_bytes(img):
    """the 2-D byte view ingest_layouts lays out"""
    return np.ascontiguousarray(img).view(np.uint8).reshape(img.shape[0], -1)


# ---- the calls ------------------------------------------------------------------------------------------------------
def set_pixels(ctx, frame, address, pitch, pixel_type, channels, on_device):
    """-> the return code (no exception: refusals are results here)"""
    return hip.load().pc_frame_set_pixels(ctx._h, frame._h, address, pitch, pixel_type, channels, on_device)


def put(ctx, frame, img, offset, pitch, where, seed):
    keep, address, pitch, on_device = il.lay_out(as_bytes(img), offset, pitch, where, seed)
    rc = set_pixels(ctx, frame, address, pitch, ref.PIXEL_TYPE[img.dtype], img.shape[2], on_device)
    return keep, rc


def run_case(ctx, kind, where, size, layouts):
    w, h, win = size
    frame = hip.Frame(ctx, w, h, win, MAX_LEVEL)
    why = ""
    try:
        for k, (offset, pitch) in enumerate(layouts):
            keep, rc = put(ctx, frame, image(kind, w, h, k & 1), offset, pitch, where, seed=2000 + k)
            try:
                why = ("set call returned %d: %s" % (rc, hip.load().pc_last_error().decode())) if rc else \
                    base.planes_mismatch(frame, expected(kind, w, h, win, k & 1))
            finally:
                if rc:
                    ctx.synchronize()
                keep.release()
            if why:
                return "offset %d pitch %d (row %d): %s" % (offset, pitch, row_bytes_of(kind, w), why)
    finally:
        frame.close()
    return why


def layout_cases():
    return [(kind, where, size) for kind in KINDS for where in il.PLACEMENTS for size in SIZES]


def layout_name(case):
    kind, where, (w, h, win) = case
    return "%s-%s-%dx%d_w%d" % (kind, where, w, h, win)


def run_layout_case(ctx, case):
    kind, where, size = case
    return run_case(ctx, kind, where, size, layouts_of(kind, size[0]))


# ---- the unfused kernels: one aligned and one misaligned layout per kind -----------------------------------------------
UNFUSED_SIZE = (66, 33, 5)


def unfused_layouts(kind):
    rb = row_bytes_of(kind, UNFUSED_SIZE[0])
    return [(0, (rb + 3) // 4 * 4), (1 if kind == "rgba8" else 2, rb + 6)]


def unfused_names():
    return ["unfused-%s" % kind for kind in KINDS]


def main():
    assert os.environ.get("POLYCHASE_PYRAMID_VARIANT") == "1", "this helper is about the kernels behind POLYCHASE_PYRAMID_VARIANT=1"
    ctx = hip.Context(0)
    for kind in KINDS:
        why = run_case(ctx, kind, "device", UNFUSED_SIZE, unfused_layouts(kind))
        print(("FAIL unfused-%s %s" % (kind, why)) if why else ("PASS unfused-%s" % kind), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
