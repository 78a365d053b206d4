#!/usr/bin/env python3
"""Case list and runner of tests/test_gray_conversion_gpu.py: frames put under a gray conversion (pc_context_set_gray_conversion)
against the numpy rule (tests/gray_conversion_ref.py) fed to the CPU oracle, bit for bit: the gray plane and, for every level, the
padded u8 plane, the derivative plane and the uint16 plane -- what a frame put with pc_frame_set_gray(reference gray) holds.

The test file runs the cases in its own process (the fused level kernel; at 23 x 19 under a 25-px window the unfused level-0
kernels) and, through main() below, once more in ONE child process under POLYCHASE_PYRAMID_VARIANT=1, which the library reads once
per process, on the unfused kernels of kernels_image.hip.  One line per case: "PASS <name>" or "FAIL <name> <what differs first>".

A case is one (size, conversion) and walks the sources (u8 RGB, float RGB, float RGBA), the placements (pageable, device) and two
layouts each -- the second with a misaligned pointer and pitch for u8, an offset and a gap for float -- on one Frame handle per
source, alternating between two images."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _ingest_check as check  # noqa: E402
import gray_conversion_ref as ref  # noqa: E402
import ingest_layouts as il  # noqa: E402
from polychase_amd import hip  # noqa: E402

MAX_LEVEL = check.MAX_LEVEL
# the level kernel's 64 x 16 tile edges and every residue of w mod 4 at window 10; 23 x 19 under a 25-px window does not fit the
# fused kernel at level 0
SIZES = [(63, 15, 10), (64, 16, 10), (65, 17, 10), (67, 35, 10), (131, 34, 10), (23, 19, 25)]
KINDS = ("rgb", "f32x3", "f32x4")
PLACEMENTS = ("pageable", "device")


@functools.lru_cache(maxsize=None)
def random_table():
    t = np.random.default_rng(20481).integers(0, 256, ref.ENTRIES, dtype=np.uint8)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def conversions():
    """name -> (weights, float table or None)"""
    return {
        "r": (ref.quantize((1, 0, 0)), None),
        "b": (ref.quantize((0, 0, 1)), None),
        "mix": (ref.quantize((0.2, 0.3, 0.5)), None),
        "srgb": (ref.DEFAULT_WEIGHTS, ref.table("srgb")),
        "random_table_mix": (ref.quantize((0.2, 0.3, 0.5)), random_table()),
    }


def cases():
    return [(size, name) for size in SIZES for name in conversions()]


def case_name(case):
    (w, h, win), name = case
    return "%s-%dx%d_w%d" % (name, w, h, win)


def case_names():
    return [case_name(c) for c in cases()]


@functools.lru_cache(maxsize=None)
def image(kind, w, h, which):
    """u8: the ingestion tests' image.  float: values over every octave of the table and beyond both ends (2^-19 .. 2^5, one in
    sixteen negative), the ingestion tests' extremes at its special pixels, and every value of ref.specials() from row 1 on"""
    if kind == "rgb":
        return check.image(kind, w, h, which)
    c = check.channels_of(kind)
    rng = np.random.default_rng([w, h, which, 77])
    img = np.exp2(rng.uniform(-19.0, 5.0, (h, w, c))).astype(np.float32)
    img[rng.integers(0, 16, (h, w, c)) == 0] *= np.float32(-1)
    ext = check._float_extremes()
    for k, (x, y) in enumerate(check.special_pixels(w, h)):
        img[y, x, :3] = ext[(3 * k + 5 * which + np.arange(3)) % len(ext)]
    sp = ref.specials()
    assert len(sp) + which <= 3 * w * (h - 2)
    for k, v in enumerate(sp):
        y, rem = divmod(3 * w + which + k, 3 * w)
        img[y, rem // 3, rem % 3] = v
    if c == 4:
        img[:, :, 3] = np.nan          # alpha must be ignored
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(kind, w, h, win, which, name):
    q, tab = conversions()[name]
    return il.expected(ref.gray(image(kind, w, h, which), q, tab if kind != "rgb" else None), win, MAX_LEVEL)


def layouts_of(kind, w):
    rb = check.row_bytes_of(kind, w)
    if kind == "rgb":
        aligned = rb + (-rb) % 4                   # the dword path of the level kernel
        return [(0, aligned), (1, aligned + 7)]    # ... and a pointer that is 1 mod 4 with a pitch that is 3 mod 4
    return [(0, rb), (4, rb + 20)]


def run_case(ctx, case, placements=PLACEMENTS):
    (w, h, win), name = case
    q, tab = conversions()[name]
    ctx.set_gray_conversion(q, tab)
    try:
        for kind in KINDS:
            frame = hip.Frame(ctx, w, h, win, MAX_LEVEL)
            try:
                k = 0
                for where in placements:
                    for offset, pitch in layouts_of(kind, w):
                        keep, rc = check.put(ctx, frame, kind, image(kind, w, h, k & 1), offset, pitch, where, seed=2000 + k)
                        try:
                            why = ("set call returned %d: %s" % (rc, hip.load().pc_last_error().decode())) if rc else \
                                check.planes_mismatch(frame, expected(kind, w, h, win, k & 1, name))
                        finally:
                            if rc:
                                ctx.synchronize()
                            keep.release()
                        if why:
                            return "%s %s offset %d pitch %d: %s" % (kind, where, offset, pitch, why)
                        k += 1
            finally:
                frame.close()
    finally:
        ctx.set_gray_conversion()
    return ""


def main():
    assert os.environ.get("POLYCHASE_PYRAMID_VARIANT") == "1", "this helper is about the kernels behind POLYCHASE_PYRAMID_VARIANT=1"
    ctx = hip.Context(0)
    for case in cases():
        why = run_case(ctx, case)
        print(("FAIL %s %s" % (case_name(case), why)) if why else ("PASS %s" % case_name(case)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
