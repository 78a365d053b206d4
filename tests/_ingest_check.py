#!/usr/bin/env python3
"""Case list and runner of tests/test_ingest_layouts_gpu.py: every source layout the C ABI accepts for a frame (base pointer,
row_pitch, placement, pixel type), through pc_frame_set_rgb / _gray / _rgb_f32, against the CPU oracle bit for bit: the gray
plane and, for every level, the padded u8 plane, the derivative plane and the uint16 plane the LK kernels read, plus the level
geometry.

The test file runs the cases in its own process (the fused level kernel) and, through main() below, once more in a child
process under POLYCHASE_PYRAMID_VARIANT=1 -- a switch the library reads once per process -- where the unfused kernels of
kernels_image.hip do the work.  One line per case: "PASS <name>" or "FAIL <name> <what differs first>".

Sizes come from the fused kernel's constants (tile 64 x 16, four pixels per lane, a 1-px halo, its edge-tile pass): both sides
of the 64- and 128-column and of the 16- and 32-row tile edges, every residue of w mod 4, two windows; 23 x 19 under a 25-px
window does not fit the fused kernel at level 0, so the unfused level-0 kernels run in the default process too.  A case is
one (pixel type, placement, size) and walks ALL its (offset, pitch) pairs on one Frame handle, alternating between two images,
so a set call that did nothing, or that left a padding byte of the previous image, shows as well."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ingest_layouts as il  # noqa: E402
from polychase_amd import hip  # noqa: E402

MAX_LEVEL = 3
SIZES = [(63, 15, 5), (64, 16, 5), (65, 17, 5), (66, 33, 5), (67, 35, 5), (67, 35, 10), (129, 18, 5), (130, 31, 5), (131, 34, 5),
         (131, 34, 10), (23, 19, 25)]                      # (w, h, window)
KINDS = ("rgb", "gray", "f32x3", "f32x4")
GPU_READ = ("device", "pinned_read", "pinned_dma")
BIG_GAP = 4100                                             # a pitch gap larger than any row here (131 x 4 floats = 2096 bytes)
PC_E_INVALID = -1


def channels_of(kind):
    return {"rgb": 3, "gray": 1, "f32x3": 3, "f32x4": 4}[kind]


def row_bytes_of(kind, w):
    return w * channels_of(kind) * (4 if kind.startswith("f32") else 1)


# ---- contents -------------------------------------------------------------------------------------------------------
def _float_extremes():
    below = np.float32(8421504.3)    # * 255 = 2^31 - 128, the last product within int32; the next float's product is 2^31
    return np.array([1.0, 0.0, 0.999999, 1.5, -0.1, 2.0, np.nan, np.inf, -np.inf, 1e10, -1e10, below,
                     np.nextafter(below, np.float32(np.inf)), -0.0, 1e-40, -below], np.float32)


def special_pixels(w, h):
    """the corners, and columns 62 .. 65 (the 64-column tile seam and its halo) of the first and the last row"""
    pos = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    pos += [(x, y) for y in (0, h - 1) for x in range(62, 66) if x < w]
    return list(dict.fromkeys(pos))


@functools.lru_cache(maxsize=None)
def image(kind, w, h, which):
    """image A (which = 0) or B (1) of a size: seeded noise, extreme pixels at special_pixels(), and for float frames every
    extreme value once more in each channel along the middle row (small images have fewer special pixels than extremes)"""
    rng = np.random.default_rng([w, h, which, KINDS.index(kind)])
    c = channels_of(kind)
    if kind in ("rgb", "gray"):
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        patterns = [(255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
        for k, (x, y) in enumerate(special_pixels(w, h)):
            img[y, x] = patterns[(k + 3 * which) % 8][:c] if kind == "rgb" else (255 if (k + which) % 2 else 0)
        img = img if kind == "rgb" else img[:, :, 0]
    else:
        img = rng.uniform(0, 1, (h, w, c)).astype(np.float32)
        ext = _float_extremes()
        for k, (x, y) in enumerate(special_pixels(w, h)):
            img[y, x, :3] = ext[(3 * k + 5 * which + np.arange(3)) % len(ext)]
        for k in range(len(ext)):
            img[h // 2, 1 + k, :3] = ext[(k + which + np.arange(3)) % len(ext)]
        if c == 4:
            img[:, :, 3] = np.nan          # alpha must be ignored
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(kind, w, h, win, which):
    return il.expected(image(kind, w, h, which), win, MAX_LEVEL)


# ---- layouts --------------------------------------------------------------------------------------------------------
def u8_gpu_layouts(rb):
    """all 16 pairs of (offset mod 4, pitch mod 4); every pitch residue once with a gap larger than a row"""
    out = []
    for o in range(4):
        for p in range(4):
            gap = (p - rb) % 4 + (BIG_GAP if o == (p + 1) % 4 else 4 * ((o + p) % 3))
            out.append((o + 8 * (p & 1), rb + gap))
    assert sorted((off % 4, pitch % 4) for off, pitch in out) == [(a, b) for a in range(4) for b in range(4)]
    assert sum(pitch - rb > rb for _, pitch in out) >= 4
    return out


def u8_pageable_layouts(rb):
    return [(o, rb + gap) for gap in (0, 1, 2, 3, 13) for o in (0, 1, 2, 3)]


def f32_layouts(rb):
    return [(o, rb + gap) for gap in (0, 4, 20, BIG_GAP) for o in (0, 4, 12)]


def layouts_of(kind, where, w):
    rb = row_bytes_of(kind, w)
    if kind.startswith("f32"):
        return f32_layouts(rb)
    return u8_pageable_layouts(rb) if where == "pageable" else u8_gpu_layouts(rb)


def layout_cases():
    return [(kind, where, size) for kind in KINDS for where in il.PLACEMENTS for size in SIZES]


def reuse_cases():
    """image A through one placement, then image B through another on the same handle with nothing in between: all ordered
    pairs, at one size per pixel type"""
    size = {"rgb": (67, 35, 5), "gray": (131, 34, 10), "f32x3": (65, 17, 5), "f32x4": (130, 31, 5)}
    return [(kind, a, b, size[kind]) for kind in KINDS for a in il.PLACEMENTS for b in il.PLACEMENTS]


def layout_name(case):
    kind, where, (w, h, win) = case
    return "%s-%s-%dx%d_w%d" % (kind, where, w, h, win)


def reuse_name(case):
    kind, a, b, (w, h, win) = case
    return "reuse-%s-%s-then-%s-%dx%d_w%d" % (kind, a, b, w, h, win)


def case_names():
    return [layout_name(c) for c in layout_cases()] + [reuse_name(c) for c in reuse_cases()]


# ---- the calls ------------------------------------------------------------------------------------------------------
def set_call(ctx, frame, kind, address, pitch, on_device):
    """the entry point of the pixel type -> its return code (no exception: refusals are results here)"""
    L = hip.load()
    if kind == "rgb":
        return L.pc_frame_set_rgb(ctx._h, frame._h, address, pitch, on_device)
    if kind == "gray":
        return L.pc_frame_set_gray(ctx._h, frame._h, address, pitch, on_device)
    return L.pc_frame_set_rgb_f32(ctx._h, frame._h, address, pitch, channels_of(kind), on_device)


def put(ctx, frame, kind, img, offset, pitch, where, seed):
    keep, address, pitch, on_device = il.lay_out(img, offset, pitch, where, seed)
    rc = set_call(ctx, frame, kind, address, pitch, on_device)
    return keep, rc


def planes_mismatch(frame, e):
    """'' when the frame's geometry and every plane equal the expected ones bit for bit, else what differs first.  The first
    download synchronises: the caller may release its source buffers afterwards."""
    got_gray = frame.gray()
    if frame.num_levels != e.num_levels:
        return "num_levels %d, expected %d" % (frame.num_levels, e.num_levels)
    if not np.array_equal(got_gray, e.gray):
        ys, xs = np.nonzero(got_gray != e.gray)
        return "gray differs at %d pixels (first x=%d y=%d: %d, expected %d)" % (len(xs), xs[0], ys[0], got_gray[ys[0], xs[0]], e.gray[ys[0], xs[0]])
    for l in range(e.num_levels):
        if frame.level_size(l) != e.sizes[l]:
            return "level %d is %s, expected %s" % (l, frame.level_size(l), e.sizes[l])
        for name, got, want in (("level", frame.level(l), e.level[l]), ("deriv", frame.deriv(l), e.deriv[l]),
                                ("level16", frame.level16(l), e.level16[l])):
            if got.shape != want.shape or got.dtype != want.dtype:
                return "%s %d is %s %s, expected %s %s" % (name, l, got.dtype, got.shape, want.dtype, want.shape)
            if not np.array_equal(got, want):
                bad = np.nonzero((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2))
                y, x = bad[0][0], bad[1][0]
                return "%s %d differs at %d positions (first padded x=%d y=%d: %s, expected %s)" % (
                    name, l, len(bad[0]), x, y, got[y, x], want[y, x])
    return ""


def run_layout_case(ctx, case):
    kind, where, (w, h, win) = case
    frame = hip.Frame(ctx, w, h, win, MAX_LEVEL)
    why = ""
    try:
        for k, (offset, pitch) in enumerate(layouts_of(kind, where, w)):
            keep, rc = put(ctx, frame, kind, image(kind, w, h, k & 1), offset, pitch, where, seed=1000 + k)
            try:
                why = ("set call returned %d: %s" % (rc, hip.load().pc_last_error().decode())) if rc else \
                    planes_mismatch(frame, expected(kind, w, h, win, k & 1))
            finally:
                if rc:
                    ctx.synchronize()
                keep.release()
            if why:
                return "offset %d pitch %d (row %d): %s" % (offset, pitch, row_bytes_of(kind, w), why)
    finally:
        frame.close()
    return why


def run_reuse_case(ctx, case):
    kind, first, second, (w, h, win) = case
    rb = row_bytes_of(kind, w)
    unit = 4 if kind.startswith("f32") else 1
    frame = hip.Frame(ctx, w, h, win, MAX_LEVEL)
    keeps = []
    try:
        ka, rca = put(ctx, frame, kind, image(kind, w, h, 0), 1 * unit, rb + 3 * unit, first, seed=31)
        keeps.append(ka)
        kb, rcb = put(ctx, frame, kind, image(kind, w, h, 1), 3 * unit, rb + 1 * unit, second, seed=32)
        keeps.append(kb)
        if rca or rcb:
            ctx.synchronize()
            return "set calls returned %d, %d: %s" % (rca, rcb, hip.load().pc_last_error().decode())
        why = planes_mismatch(frame, expected(kind, w, h, win, 1))
        if why:
            return why
        # ... and back: A through the second placement over B's planes
        kc, rcc = put(ctx, frame, kind, image(kind, w, h, 0), 0, rb, second, seed=33)
        keeps.append(kc)
        if rcc:
            ctx.synchronize()
            return "third set call returned %d" % rcc
        return planes_mismatch(frame, expected(kind, w, h, win, 0))
    finally:
        ctx.synchronize()
        for k in keeps:
            k.release()
        frame.close()


def run_all(ctx, report):
    for case in layout_cases():
        report(layout_name(case), run_layout_case(ctx, case))
    for case in reuse_cases():
        report(reuse_name(case), run_reuse_case(ctx, case))


def main():
    assert os.environ.get("POLYCHASE_PYRAMID_VARIANT") == "1", "this helper is about the kernels behind POLYCHASE_PYRAMID_VARIANT=1"
    ctx = hip.Context(0)
    run_all(ctx, lambda name, why: print(("FAIL %s %s" % (name, why)) if why else ("PASS %s" % name), flush=True))
    ctx.close()


if __name__ == "__main__":
    main()
