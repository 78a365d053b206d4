"""GPU: frame ingestion -- every source layout the C ABI accepts (base pointer, row_pitch, placement, pixel type) through
pc_frame_set_rgb / _gray / _rgb_f32, against the CPU oracle.  Everything is bit-exact; nothing is a tolerance.

  * tests/_ingest_check.py has the case list and what a case compares (gray; per level the padded u8 plane, the derivative plane
    and the uint16 plane of Frame.level16; num_levels and level_size).  The cases run here on the fused level kernel (and, at
    23 x 19 under a 25-px window, on the unfused level-0 kernels) and once more in ONE child process under
    POLYCHASE_PYRAMID_VARIANT=1, which the library reads once per process, on the unfused kernels of kernels_image.hip;
  * calls the entry points must refuse (PC_E_INVALID), leaving the frame's planes as they were;
  * widths with w mod 4 = 1, 2, 3 through the pipelined analyzer with device frames (an unaligned device pitch through
    pc_analyzer_put_frame) and through polychase_core (PC_FRAME_PINNED_HOST into the two staging buffers of the copy stream, at an
    unaligned pitch), u8 and float32 RGBA, against the reference-shaped CPU path record for record."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ingest_check as check
import ingest_layouts as il
import oracle
from polychase_amd import hip, synth
from test_core_gpu import _dump, _expect, core  # noqa: F401  (core is the module fixture that imports polychase_core)
from test_gpu_parity import _compare_clip

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


# ---- the layouts, fused kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", check.layout_cases(), ids=check.layout_name)
def test_planes_of_every_layout_match_the_oracle(ctx, case):
    assert os.environ.get("POLYCHASE_PYRAMID_VARIANT", "0") == "0", "this process must run the fused level kernel"
    assert check.run_layout_case(ctx, case) == ""


@pytest.mark.parametrize("case", check.reuse_cases(), ids=check.reuse_name)
def test_a_reused_frame_holds_the_second_image(ctx, case):
    assert check.run_reuse_case(ctx, case) == ""


def test_the_case_list_covers_what_it_claims():
    """every (offset mod 4, pitch mod 4) at every size -- hence at every residue of w mod 4 -- for the GPU-read placements;
    every gap and offset of the pageable and the float lists at every size; gaps larger than a row; the sizes themselves"""
    assert {w % 4 for w, _, _ in check.SIZES} == {0, 1, 2, 3}
    assert {(w, h) for w, h, _ in check.SIZES} >= {(63, 15), (64, 16), (65, 17), (66, 33), (67, 35), (129, 18), (130, 31), (131, 34), (23, 19)}
    assert {(67, 35, 5), (67, 35, 10), (131, 34, 5), (131, 34, 10), (23, 19, 25)} <= set(check.SIZES)
    cases = check.layout_cases()
    for kind in check.KINDS:
        for where in il.PLACEMENTS:
            assert [s for k, p, s in cases if (k, p) == (kind, where)] == check.SIZES
    for w, _, _ in check.SIZES:
        for kind in ("rgb", "gray"):
            rb = check.row_bytes_of(kind, w)
            for where in check.GPU_READ:
                lay = check.layouts_of(kind, where, w)
                assert {(o % 4, p % 4) for o, p in lay} == {(a, b) for a in range(4) for b in range(4)}
                assert any(p - rb > rb for _, p in lay)
            lay = check.layouts_of(kind, "pageable", w)
            assert {p - rb for _, p in lay} == {0, 1, 2, 3, 13} and {o for o, _ in lay} == {0, 1, 2, 3}
        for kind in ("f32x3", "f32x4"):
            rb = check.row_bytes_of(kind, w)
            for where in il.PLACEMENTS:
                lay = check.layouts_of(kind, where, w)
                assert {o for o, _ in lay} == {0, 4, 12} and {p - rb for _, p in lay} == {0, 4, 20, check.BIG_GAP} and check.BIG_GAP > rb
    assert len(check.reuse_cases()) == 4 * 16
    # the contents: every float extreme occurs in every float image, alpha is NaN throughout
    ext = check._float_extremes()
    assert np.isnan(ext).sum() == 1 and np.isinf(ext).sum() == 2 and len(ext) == 16
    for w, h, _ in check.SIZES:
        for which in (0, 1):
            for kind in ("f32x3", "f32x4"):
                img = check.image(kind, w, h, which)
                bits = set(img[:, :, :3].view(np.uint32).ravel().tolist())
                assert set(ext.view(np.uint32).tolist()) <= bits
                assert kind == "f32x3" or np.isnan(img[:, :, 3]).all()
            rgb = check.image("rgb", w, h, which)
            assert all(set(rgb[y, x].tolist()) <= {0, 255} for x, y in check.special_pixels(w, h))
    for w, h, win in check.SIZES:
        for kind in check.KINDS:   # the two images of a size differ in every plane a stale one could hide in
            a, b = check.expected(kind, w, h, win, 0), check.expected(kind, w, h, win, 1)
            assert not np.array_equal(a.gray, b.gray) and not np.array_equal(a.level16[-1], b.level16[-1])


# ---- the same cases on the unfused kernels --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unfused_lines():
    env = dict(os.environ)
    env["POLYCHASE_PYRAMID_VARIANT"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_ingest_check.py")], env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, f"the helper failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", check.case_names())
def test_unfused_kernels_match_the_oracle(unfused_lines, name):
    """among them rgb-device-64x16_w5: a width that is a multiple of 4 behind a misaligned device pointer, where
    launch_rgb2gray's own alignment test picks the one-pixel-per-lane kernel"""
    mine = [l for l in unfused_lines if l.split()[1:2] == [name]]
    assert mine == [f"PASS {name}"], mine


def test_the_unfused_list_has_the_misaligned_pointer_at_a_width_that_is_a_multiple_of_four():
    lay = check.layouts_of("rgb", "device", 64)
    assert ("rgb", "device", (64, 16, 5)) in check.layout_cases()
    assert any(o % 4 == 1 and p % 4 == 0 for o, p in lay) and any(o % 4 == 0 and p % 4 == 0 for o, p in lay)


# ---- refusals -------------------------------------------------------------------------------------------------------
def _refused(ctx, frame, kind, buf, address_offset, pitch, channels):
    """pageable host memory (on_device = 0) large enough for the call: were it not refused, it would read valid memory"""
    L, on_device = hip.load(), 0
    address = buf.ctypes.data + address_offset
    if kind == "rgb":
        rc = L.pc_frame_set_rgb(ctx._h, frame._h, address, pitch, on_device)
    elif kind == "gray":
        rc = L.pc_frame_set_gray(ctx._h, frame._h, address, pitch, on_device)
    else:
        rc = L.pc_frame_set_rgb_f32(ctx._h, frame._h, address, pitch, channels, on_device)
    return rc


@pytest.mark.parametrize("kind", check.KINDS)
def test_refused_calls_leave_the_planes_intact(ctx, kind):
    w, h, win = 67, 35, 5
    frame = hip.Frame(ctx, w, h, win, check.MAX_LEVEL)
    keep, rc = check.put(ctx, frame, kind, check.image(kind, w, h, 0), 0, check.row_bytes_of(kind, w), "pageable", seed=1)
    assert rc == 0
    e = check.expected(kind, w, h, win, 0)
    assert check.planes_mismatch(frame, e) == ""
    rb = check.row_bytes_of(kind, w)
    # room for the widest call below (5 float channels, full pitch), so that a call that is NOT refused reads nothing outside
    buf = np.random.default_rng(9).integers(0, 256, 16 + h * w * 5 * 4, dtype=np.uint8)
    assert buf.ctypes.data % 4 == 0
    ch = check.channels_of(kind)
    calls = [("row_pitch = row_bytes - 1", 0, rb - 1, ch)]
    if kind.startswith("f32"):
        calls += [("row_pitch = row_bytes - 4", 0, rb - 4, ch), ("pitch % 4 == 2", 0, rb + 2, ch), ("pointer off by 2", 2, rb, ch),
                  ("2 channels", 0, w * 2 * 4, 2), ("5 channels", 0, w * 5 * 4, 5)]
    for what, off, pitch, channels in calls:
        rc = _refused(ctx, frame, kind, buf, off, pitch, channels)
        assert rc == check.PC_E_INVALID, (what, rc)
        assert check.planes_mismatch(frame, e) == "", what
    keep.release()
    frame.close()


# ---- through the analyzer and the product ---------------------------------------------------------------------------
WIDTHS = [157, 158, 159]     # w mod 4 = 1, 2, 3: 3 * w is no multiple of 4, every pitch of a contiguous frame is unaligned
CLIP_H, CLIP_N = 93, 10


_clips = {}


def _clip(w):
    if w not in _clips:
        clip = synth.NoiseClip(w, CLIP_H, CLIP_N)
        frames = [clip.frame(t) for t in range(CLIP_N)]
        _clips[w] = (frames, oracle.analyze_clip(frames, first_frame=1, threads=4))
    return _clips[w]


@pytest.mark.parametrize("w", WIDTHS)
def test_analyzer_with_device_frames_at_an_unaligned_pitch(ctx, w):
    import torch
    from polychase_amd.pipeline import ClipAnalyzer
    frames, (kps_o, flows_o) = _clip(w)
    assert (3 * w) % 4 != 0 and hip.flow_options().window_size == 10
    got_kps, got_flows = {}, {}

    def sink(f1, kps, detected, flows):
        assert detected
        got_kps[f1] = kps
        for f2, rec in flows.items():
            got_flows[(f1, f2)] = rec

    an = ClipAnalyzer(ctx, w, CLIP_H, 1, CLIP_N, lambda fid: torch.from_numpy(frames[fid - 1]).cuda())
    an.run(range(1, 1 + CLIP_N), sink)
    an.close()
    assert min(len(k) for k in kps_o.values()) > 20 and len(flows_o) > 4 * CLIP_N
    _compare_clip(kps_o, flows_o, got_kps, got_flows)


@pytest.mark.parametrize("pixels", ["u8", "f32_rgba"])
@pytest.mark.parametrize("w", WIDTHS)
def test_product_with_host_frames_at_an_unaligned_pitch(core, tmp_path, w, pixels):
    frames, _ = _clip(w)
    given = frames
    if pixels == "f32_rgba":
        rng = np.random.default_rng(w)
        given = []
        for f in frames:
            x = (f.astype(np.float32) + rng.uniform(0.05, 0.95, f.shape).astype(np.float32)) / np.float32(255.0)
            given.append(np.ascontiguousarray(np.concatenate([x, np.full(f.shape[:2] + (1,), np.nan, np.float32)], axis=2)))
            assert np.array_equal(il.float_to_u8(given[-1][:, :, :3]), f)
    path = str(tmp_path / f"{pixels}_{w}.db")
    stats = core.generate_optical_flow_database(core.VideoInfo(w, CLIP_H, 1, CLIP_N), lambda fid: given[fid - 1], None, path)
    assert stats.frames_processed == CLIP_N
    ek, ef = _expect(frames, 1)
    k, f = _dump(path)
    assert len(ek) == CLIP_N and k == ek
    assert f == ef
