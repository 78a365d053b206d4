#!/usr/bin/env python3
"""raycast_bench.py -- batched closest-hit ray casting (pc_raycast_pixels, the tracker's K12): LBVH vs the
exhaustive sweep, and the LBVH build time, on a wavy grid mesh.   python tools/raycast_bench.py [--grid 700] [--rays 40000]

--render W H [--margin M]: the mesh render (pc_mesh_render) of a W x H frame -- mask only, and all three planes, into device
memory -- beside pc_raycast_pixels over the same W * H pixels in linear order, on the wavy grid (--grid) and on the benchmark's C5
mesh (the two-triangle plane of tests/c5_endtoend.py).  Wall clock per call here (launch + the call's synchronisation; the pixel
list's also has its transfers).  Device time of every launch: run the same command under `rocprofv3 --kernel-trace
--output-format csv -d DIR --`, then `--render W H --from-trace DIR` (same --warmup / --repeats) groups the trace's dispatches by
mesh and by the planes asked for and writes their medians into profiles/mesh_render.json.  (The call synchronises its stream
before it returns, so HIP events recorded around it from outside would time the host's part too; the trace times the kernels.)"""
import argparse, csv, ctypes as C, glob, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))

PROFILE = os.path.join(ROOT, "profiles", "mesh_render.json")
RENDER_KERNELS = ("mesh_render_kernel", "raycast_bvh_kernel", "mask_choke_kernel")


def _update_profile(key, value):
    doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
    doc[key] = value
    json.dump(doc, open(PROFILE, "w"), indent=1)


def _fold_trace(a):
    """the per-dispatch rows of a rocprofv3 kernel trace of `--render` (same --warmup / --repeats) -> the profile: device time of
    every launch, grouped by mesh and by what the call asked for, in the order _render_bench makes the calls; warm-ups dropped"""
    import statistics
    rows = []
    for path in glob.glob(os.path.join(a.from_trace, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    by = {k: [us for _, name, us in rows if k in name] for k in RENDER_KERNELS}
    per_call, n_list = a.warmup + a.repeats, 1 + max(2, a.repeats // 5)
    assert len(by["mesh_render_kernel"]) == 2 * 3 * per_call and len(by["raycast_bvh_kernel"]) == 2 * n_list, \
        (len(by["mesh_render_kernel"]), len(by["raycast_bvh_kernel"]))

    def stat(v):
        return {"launches": len(v), "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}

    out = {}
    for k, mesh in enumerate(("grid", "c5_plane")):
        res = {}
        for j, label in enumerate(("mask_only", "mask_margin", "three_planes")):
            at = (3 * k + j) * per_call
            res[label] = stat(by["mesh_render_kernel"][at + a.warmup:at + per_call])
        res["pixel_list_raycast_bvh_kernel"] = stat(by["raycast_bvh_kernel"][k * n_list + 1:(k + 1) * n_list])
        res["mask_only_over_pixel_list"] = res["mask_only"]["median_us"] / res["pixel_list_raycast_bvh_kernel"]["median_us"]
        out[mesh] = res
    out["mask_choke_kernel"] = stat(by["mask_choke_kernel"])
    tag = f"device_{a.render[0]}x{a.render[1]}" + (f"_{a.tag}" if a.tag else "")
    _update_profile(tag, out)
    print(json.dumps({tag: out}))


def _render_bench(a):
    import numpy as np
    import torch
    import refine_scene as S
    from polychase_amd import hip
    w, h = a.render
    L = hip.load()
    VP = C.c_void_p

    class RayCamera(C.Structure):
        _fields_ = [("dir_matrix", C.c_float * 9), ("origin", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                    ("cx", C.c_float), ("cy", C.c_float), ("unproject_sign", C.c_float)]

    L.pc_mesh_create.argtypes = [VP, VP, C.c_int, VP, C.c_int, C.POINTER(VP)]
    L.pc_mesh_destroy.argtypes = [VP]
    L.pc_mesh_render.argtypes = [VP, VP, C.POINTER(RayCamera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP, VP, VP]
    L.pc_raycast_pixels.argtypes = [VP, VP, C.POINTER(RayCamera), VP, C.c_int, C.c_int, VP, VP, VP, VP]
    ctx = hip.Context(0)
    # a camera 6 units in front of the mesh (4 units wide), looking at it: the mesh fills about half the frame's height
    f = 0.75 * h
    cam = RayCamera()
    cam.dir_matrix[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    cam.origin[:] = [0.0, 0.0, -6.0]
    cam.fx = cam.fy = f
    cam.cx, cam.cy, cam.unproject_sign = w / 2, h / 2, 1.0
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    xy = np.stack([px.ravel(), py.ravel()], 1).astype(np.float32)
    n = w * h
    meshes = {"grid": S.grid_mesh(a.grid),
              "c5_plane": (np.array([[-2, -1.125, 0], [2, -1.125, 0], [2, 1.125, 0], [-2, 1.125, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32))}
    out = {"frame": [w, h], "margin": a.margin, "repeats": a.repeats, "lib": os.environ.get("POLYCHASE_HIP_LIB", "default")}
    d_prim = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_depth = torch.empty(n, dtype=torch.float32, device="cuda:0")
    d_mask = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for name, (verts, tris) in meshes.items():
        verts, tris = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.uint32)
        m = VP()
        assert L.pc_mesh_create(ctx._h, verts.ctypes.data_as(VP), len(verts), tris.ctypes.data_as(VP), len(tris), C.byref(m)) == 0
        res = {"triangles": len(tris)}
        for label, planes, margin in (("mask_only", (None, None, VP(d_mask.data_ptr())), 0), ("mask_margin", (None, None, VP(d_mask.data_ptr())), a.margin),
                                      ("three_planes", (VP(d_prim.data_ptr()), VP(d_depth.data_ptr()), VP(d_mask.data_ptr())), 0)):
            times = []
            for k in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                assert L.pc_mesh_render(ctx._h, m, C.byref(cam), w, h, 1, 0, margin, 1, *planes) == 0, L.pc_last_error()
                times.append(time.perf_counter() - t0)
            t = np.array(times[a.warmup:]) * 1e6
            res[label] = {"wall_us_median": float(np.median(t)), "wall_us_min": float(t.min())}
        res["covered"] = float((d_mask != 0).float().mean().item())
        hit, pos = np.empty(n, np.uint8), np.empty((n, 3), np.float32)
        prim, uvt = np.empty(n, np.uint32), np.empty((n, 3), np.float32)
        times = []
        for k in range(1 + max(2, a.repeats // 5)):
            t0 = time.perf_counter()
            assert L.pc_raycast_pixels(ctx._h, m, C.byref(cam), xy.ctypes.data_as(VP), n, 1, hit.ctypes.data_as(VP), pos.ctypes.data_as(VP),
                                       prim.ctypes.data_as(VP), uvt.ctypes.data_as(VP)) == 0
            times.append(time.perf_counter() - t0)
        res["pixel_list"] = {"wall_us_median": float(np.median(np.array(times[1:]) * 1e6)), "bytes_up": int(xy.nbytes),
                             "bytes_down": int(hit.nbytes + pos.nbytes + prim.nbytes + uvt.nbytes)}
        assert np.array_equal(hit != 0, (d_mask != 0).cpu().numpy()) or a.margin < 0
        L.pc_mesh_destroy(m)
        out[name] = res
    ctx.close()
    tag = f"wall_{w}x{h}" + (f"_{a.tag}" if a.tag else "")
    if not a.no_profile:
        _update_profile(tag, out)
    print(json.dumps({tag: out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=700)
    ap.add_argument("--rays", type=int, default=40000)
    ap.add_argument("--render", type=int, nargs=2, metavar=("W", "H"))
    ap.add_argument("--margin", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--tag", default="")
    ap.add_argument("--from-trace", default=None)
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    if a.render and a.from_trace:
        return _fold_trace(a)
    if a.render:
        return _render_bench(a)
    import numpy as np
    import torch  # noqa: F401
    import polychase_core as core
    import refine_scene as S
    verts, tris = S.grid_mesh(a.grid)
    t0 = time.perf_counter(); mesh = core.AcceleratedMesh(verts, tris); t_build = time.perf_counter() - t0
    t0 = time.perf_counter(); mesh = core.AcceleratedMesh(verts, tris); t_build = min(t_build, time.perf_counter() - t0)
    cam = S.true_camera(3)
    view = np.eye(4, dtype=np.float32); view[:3, :3], view[:3, 3] = cam.R(), cam.t
    intr = core.CameraIntrinsics(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, aspect_ratio=1.0, width=S.W, height=S.H,
                                 convention=core.CameraConvention.OpenGL)
    st = core.SceneTransformations(np.eye(4, dtype=np.float32), view, intr)
    xy = np.random.default_rng(0).uniform([0, 0], [S.W, S.H], (a.rays, 2)).astype(np.float32)
    res = {}
    for name, ex in (("lbvh", False), ("sweep", True)):
        core._ray_cast_pixels(mesh, st, xy[:64], True, ex)
        t0 = time.perf_counter(); h = core._ray_cast_pixels(mesh, st, xy, True, ex); res[name] = (time.perf_counter() - t0, sum(x is not None for x in h))
    print(f"{len(tris)} triangles, {a.rays} rays: mesh upload + LBVH build {t_build * 1e3:.1f} ms; "
          + "; ".join(f"{k} {v[0] * 1e3:.1f} ms ({v[1]} hits)" for k, v in res.items()) + "  (times include H2D/D2H and Python object creation)")

if __name__ == "__main__":
    main()
