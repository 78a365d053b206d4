#!/usr/bin/env python3
"""Frame ingestion through polychase_core: host frames as uint8 RGB, as Blender's float32 RGBA and as
scene-linear float32 RGB (the uint8 clip through the sRGB EOTF: what an EXR plate holds), or device-resident uint8 RGB
(uint8_rgb_device: no transfer at all, the GPU side of ingestion alone), no database.  uint8_rgba (the same bytes with an alpha
channel), uint16_rgb (x * 257) and float16_rgba (the float32 RGBA clip rounded to half) are the same pictures in the pixel types
a decoder, a 16-bit plate and an EXR hand out: converted on the GPU like the others, so the clips differ in bytes moved only.
`POLYCHASE_COPY_THREADS=1` gives the single-threaded copy for comparison.

    python tools/ingest_bench.py [--config c2] [--frames 120] [--clips uint8_rgb,float32_rgba,float32_rgb_linear,uint8_rgb_device,uint8_rgba,uint16_rgb,float16_rgba]
                                 [--channel-weights R G B] [--float-transfer none|srgb|gamma] [--float-gamma G] [--float-exposure STOPS]
                                 [--lens-k1 K]

The last four are OpticalFlowOptions' gray conversion (channel_weights, float_transfer, float_transfer_gamma, float_exposure) of
every run; --lens-k1 K is OpticalFlowOptions.lens = LensModel(fx = fy = width, centred principal point, k1 = K): every frame is
undistorted as it is put; --repeat N times every clip N times and reports the median with min and max beside it.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))

CLIPS = ("uint8_rgb", "float32_rgba", "float32_rgb_linear", "uint8_rgb_device", "uint8_rgba", "uint16_rgb", "float16_rgba")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--clips", default="uint8_rgb,float32_rgba")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--channel-weights", type=float, nargs=3, default=None, metavar=("R", "G", "B"))
    ap.add_argument("--float-transfer", choices=["none", "srgb", "gamma"], default="none")
    ap.add_argument("--float-gamma", type=float, default=2.2)
    ap.add_argument("--float-exposure", type=float, default=0.0)
    ap.add_argument("--lens-k1", type=float, default=None, metavar="K")
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401
    import polychase_core as core
    from polychase_amd import synth

    names = [c for c in a.clips.split(",") if c]
    assert set(names) <= set(CLIPS), names
    w, h, ml = {"c2": (1920, 1080, 3), "c3": (3840, 2160, 4)}[a.config]
    clip = synth.NoiseClip(w, h, 24)
    u8 = [clip.frame(t) for t in range(24)]
    clips = {"uint8_rgb": u8}
    if "float32_rgba" in names:
        clips["float32_rgba"] = [np.concatenate([x.astype(np.float32) / 255.0, np.ones((h, w, 1), np.float32)], axis=2) for x in u8[:12]]
    if "uint8_rgba" in names:
        clips["uint8_rgba"] = [np.concatenate([x, np.full((h, w, 1), 255, np.uint8)], axis=2) for x in u8]
    if "uint16_rgb" in names:
        clips["uint16_rgb"] = [x.astype(np.uint16) * np.uint16(257) for x in u8[:12]]
    if "float16_rgba" in names:
        clips["float16_rgba"] = [np.concatenate([x.astype(np.float32) / 255.0, np.ones((h, w, 1), np.float32)], axis=2).astype(np.float16)
                                 for x in u8[:12]]
    if "float32_rgb_linear" in names:
        c = np.arange(256) / 255.0
        eotf = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(np.float32)
        clips["float32_rgb_linear"] = [np.ascontiguousarray(eotf[x]) for x in u8[:12]]
    if "uint8_rgb_device" in names:
        import torch
        clips["uint8_rgb_device"] = [torch.from_numpy(x).cuda() for x in u8]
        torch.cuda.synchronize()
    fo = core.OpticalFlowOptions()
    fo.max_level = ml
    if a.lens_k1 is not None:
        fo.lens = core.LensModel(float(w), float(w), (w - 1) / 2.0, (h - 1) / 2.0, k1=a.lens_k1)
    fo.channel_weights = tuple(a.channel_weights) if a.channel_weights else None
    fo.float_transfer = a.float_transfer
    fo.float_transfer_gamma = a.float_gamma
    fo.float_exposure = a.float_exposure
    vi = core.VideoInfo(w, h, 1, a.frames)
    out = {"config": a.config, "frames": a.frames, "copy_threads": os.environ.get("POLYCHASE_COPY_THREADS", "default")}
    if a.channel_weights:
        out["channel_weights"] = a.channel_weights
    if a.float_transfer != "none":
        out["float_transfer"] = {"kind": a.float_transfer, "gamma": a.float_gamma, "exposure": a.float_exposure}
    if a.lens_k1 is not None:
        out["lens_k1"] = a.lens_k1
    for name in names:
        frames = clips[name]
        n = len(frames)

        def acc(fid):
            t = (fid - 1) % (2 * n - 2)
            return frames[t if t < n else 2 * n - 2 - t]
        core.generate_optical_flow_database(core.VideoInfo(w, h, 1, 20), acc, None, "", core.GFTTOptions(), fo)   # warm-up
        fps, fps_run, setup = [], [], []
        for _ in range(max(1, a.repeat)):
            t0 = time.perf_counter()
            st = core.generate_optical_flow_database(vi, acc, None, "", core.GFTTOptions(), fo)
            dt = time.perf_counter() - t0
            fps.append(a.frames / dt)
            fps_run.append(a.frames / (dt - st.seconds_setup))   # without the per-run set-up (engine, lens map)
            setup.append(st.seconds_setup)
        med = statistics.median(fps)
        nbytes = frames[0].nbytes if hasattr(frames[0], "nbytes") else frames[0].numel() * frames[0].element_size()
        out[name] = {"fps": med, "host_GBps": med * nbytes / 1e9}
        out[name].update(fps_without_setup=statistics.median(fps_run), seconds_setup=statistics.median(setup))
        if a.repeat > 1:
            out[name].update(fps_min=min(fps), fps_max=max(fps), runs=len(fps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
