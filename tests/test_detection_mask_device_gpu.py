"""GPU: the detection mask handed over as device memory (on_device = 1: a torch CUDA uint8 tensor, packed or pitched) through
pc_frame_set_mask and pc_analyzer_set_mask, pc_analyzer_set_mask's own refusals, and the launches of a context that never sees
a mask.  References as in tests/test_detection_mask_gpu.py (tests/masked_gftt_ref.py)."""
import functools

import numpy as np
import pytest

import masked_gftt_ref as ref
import oracle
from polychase_amd import hip, synth
from polychase_amd.pipeline import ClipAnalyzer

pytestmark = pytest.mark.gpu

W, H, N = 320, 240, 12


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


def _device_mask(torch, m, pad):
    """the mask as a CUDA tensor; pad > 0: a view of a wider tensor whose other bytes say "on" (reading them would show)"""
    h, w = m.shape
    wide = torch.full((h, w + pad), 255, dtype=torch.uint8, device="cuda")
    wide[:, :w] = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    return wide[:, :w]


@pytest.mark.parametrize("pad", [0, 13], ids=["packed", "pitched"])
@pytest.mark.parametrize("size", [(333, 211), (320, 200)], ids=lambda s: "%dx%d" % s)
def test_frame_mask_from_device_memory(torch, ctx, size, pad):
    w, h = size
    g = ref.test_image(w, h)
    m = ref.mask_column_and_disc(w, h)
    ekps, eeig, encand = ref.gftt(g, oracle.gftt_options(), m)      # a new context: the default arithmetic = the default emulation
    dm = _device_mask(torch, m, pad)
    assert dm.is_contiguous() == (pad == 0)
    f = hip.Frame(ctx, w, h)
    f.set_gray(g)
    f.set_mask(dm)
    f.detect()
    assert f.num_candidates == encand
    assert np.array_equal(f.keypoints(), ekps)
    assert np.array_equal(f.min_eig().view(np.uint32), eeig.view(np.uint32))
    f.close()


def test_mask_tensor_whose_rows_are_not_contiguous_is_refused(torch, ctx):
    f = hip.Frame(ctx, W, H)
    t = torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        f.set_mask(t[:, ::2])                                       # right shape and dtype, a byte skipped between pixels
    with pytest.raises(ValueError):
        f.set_mask(torch.zeros((W, H), dtype=torch.uint8, device="cuda").t())   # rows closer than the width
    f.close()


@functools.lru_cache(maxsize=None)
def _clip():
    c = synth.NoiseClip(W, H, N)
    return [c.frame(i) for i in range(N)]


def _moving_mask(fid):
    m = np.zeros((H, W), np.uint8)
    m[20 + 5 * fid:150 + 5 * fid, 15 * fid:120 + 15 * fid] = (1, 128, 255)[fid % 3]
    return m


def test_analyzer_mask_from_device_memory_lives_until_its_frames_are_ingested(torch, ctx):
    """every frame is put under a device mask of its own (odd frames pitched) that the caller drops at once: the wrapper holds
    it for the slot, and a later set_mask does not reach the detections already enqueued"""
    frames = _clip()
    an = hip.Analyzer(ctx, W, H)
    for fid in range(1, N + 1):
        an.set_mask(_device_mask(torch, _moving_mask(fid), 13 * (fid % 2)))
        an.put_frame(fid, frames[fid - 1], will_detect=True)
    an.set_mask(torch.zeros((H, W), dtype=torch.uint8, device="cuda"))
    got = {}
    for fid in range(1, N + 1):
        an.submit(fid, [])
        r = an.collect()
        got[r[0]] = r[1].copy()
    an.close()
    for fid in range(1, N + 1):
        ekps = ref.gftt(oracle.rgb2gray(frames[fid - 1]), oracle.gftt_options(), _moving_mask(fid))[0]
        assert np.array_equal(got[fid], ekps), fid


def test_analyzer_set_mask_refuses_a_row_pitch_below_the_width(torch, ctx):
    an = hip.Analyzer(ctx, W, H)
    m = np.zeros((H, W), np.uint8)
    dm = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    L = hip.load()
    assert L.pc_analyzer_set_mask(an._h, m.ctypes.data, W - 1, 0) != 0
    assert L.pc_analyzer_set_mask(an._h, dm.data_ptr(), W - 1, 1) != 0
    with pytest.raises(hip.PolychaseHipError):
        hip._check(L.pc_analyzer_set_mask(an._h, m.ctypes.data, W - 1, 0))
    # refused calls leave the analyzer without a mask
    an.put_frame(1, _clip()[0], will_detect=True)
    an.submit(1, [])
    assert np.array_equal(an.collect()[1], oracle.gftt(oracle.rgb2gray(_clip()[0])))
    an.close()


# Launches per kernel class (pc_context_get_timing) of 20 pipelined steps of a 320x240 clip on a context that never sees a mask,
# recorded from the commit before the detection mask existed: the mask must add no launch to such a context.
LAUNCHES_OF_20_UNMASKED_STEPS = {"gray": 0, "pyramid": 40, "min_eig": 20, "nms": 20, "sort": 20, "suppress": 20, "lk": 20, "compact": 20,
                                 "lk_fb": 0}


def _launches(ctx, mask):
    clip = synth.NoiseClip(W, H, 48)
    frames = [clip.frame(i) for i in range(48)]
    an = ClipAnalyzer(ctx, W, H, 1, 48, lambda f: frames[f - 1])
    if mask is not None:
        an.an.set_mask(mask)
    an.run(range(9, 13), None)
    ctx.synchronize()
    ctx.enable_timing(True)
    ctx.reset_timing()
    an.run(range(13, 33), None)
    counts = {k: v[0] for k, v in ctx.timing().items()}
    ctx.enable_timing(False)
    an.close()
    return counts


def test_a_context_that_never_sees_a_mask_enqueues_the_launches_of_before():
    c = hip.Context(0)
    counts = _launches(c, None)
    c.close()
    print("launches of 20 unmasked steps:", counts)
    assert counts == LAUNCHES_OF_20_UNMASKED_STEPS


def test_a_mask_adds_no_launch_either():
    """the masked kernels replace the unmasked ones one for one; the mask's copy is not a kernel"""
    c = hip.Context(0)
    counts = _launches(c, np.full((H, W), 255, np.uint8))
    c.close()
    print("launches of 20 masked steps:", counts)
    assert counts == LAUNCHES_OF_20_UNMASKED_STEPS
