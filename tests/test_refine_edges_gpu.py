"""GPU: the refiner's two sweep kernels at the C ABI -- pc_refine_total_cost, pc_refine_normal_equations -- against the float64
restatement of tests/refiner_ref.py, entry by entry and off the one family of scenes tests/test_refiner_gpu.py feeds them.
Every one of the (2B)(2B+1)/2 + 2B values of every edge, every per-edge cost and the total are held to
    |gpu - float64| <= 4 * rho * 2^-24 * A_k,   A_k = sum_i |term_i| / n_valid,
with rho the worst noise of the float32 restatement over this file's cases (measured in tests/test_refiner_ref_cpu.py, recorded
in profiles/refiner_edge_noise.txt); a value whose A_k is 0 has to be exactly 0, and edge_valid has to be equal: every keypoint
is constructed so that float32 cannot choose another triangle.  Named cases (refiner_ref.case_specs): model matrices that are
not their own transpose x both conventions x aspect ratios x losses x intrinsics flags, edges of 0 .. 1025 residuals around the
wave width and the kernels' strides, invalid residuals, a target camera that looks away, the triangle cache across sweeps, the
normal equations before any cost sweep, a cached triangle kept behind a nearer one; one scene goes through polychase_core and
holds the host's assembly to the same bound."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

from polychase_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refiner_ref as rr  # noqa: E402
import tracker_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
VP = C.c_void_p
SPECS = rr.case_specs()
WORST = {"triangle": 0.0, "gradient": 0.0, "edge cost": 0.0, "total cost": 0.0, "assembled JtJ": 0.0, "assembled Jtr": 0.0}


class RefineDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int), ("n_edges", C.c_int), ("kp_offset", VP), ("kp_xy", VP), ("edge_src", VP), ("edge_tgt", VP),
                ("edge_offset", VP), ("res_src_kp", VP), ("res_tgt_xy", VP), ("edge_weight", VP), ("model_matrix", C.c_float * 16),
                ("model_matrix_inv", C.c_float * 16), ("block_len", C.c_int), ("optimize_focal_length", C.c_int),
                ("optimize_principal_point", C.c_int)]


class RefineCamera(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("aspect_ratio", C.c_float), ("unproject_sign", C.c_float), ("reserved", C.c_float * 2)]


def _p(a):
    return a.ctypes.data_as(VP)


@pytest.fixture(scope="module")
def env():
    L = hip.load()
    ctx = hip.Context(0)
    L.pc_mesh_create.argtypes = [VP, VP, C.c_int, VP, C.c_int, C.POINTER(VP)]
    L.pc_mesh_destroy.argtypes = [VP]
    L.pc_refine_problem_create.argtypes = [VP, VP, C.POINTER(RefineDesc), C.POINTER(VP)]
    L.pc_refine_total_cost.argtypes = [VP, VP, C.POINTER(RefineCamera), C.c_int, C.c_float, C.POINTER(C.c_double)]
    L.pc_refine_normal_equations.argtypes = [VP, VP, C.POINTER(RefineCamera), C.c_int, C.c_float, VP, VP]
    L.pc_refine_problem_destroy.argtypes = [VP]
    meshes = {}
    for kind, (verts, tris) in (("grid", tr.grid_mesh()), ("two", rr.two_triangle_mesh())):
        verts, tris = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.uint32)
        m = VP()
        assert L.pc_mesh_create(ctx._h, _p(verts), len(verts), _p(tris), len(tris), C.byref(m)) == 0, L.pc_last_error()
        meshes[kind] = m
    yield L, ctx, meshes
    for m in meshes.values():
        L.pc_mesh_destroy(m)
    ctx.close()
    print("\nworst |gpu - float64| / bound:", {k: round(v, 4) for k, v in WORST.items()})


@pytest.fixture(scope="module")
def rho():
    return rr.rho_worst()


def _abi_cameras(cams):
    out = (RefineCamera * len(cams))()
    for f, c in enumerate(cams):
        out[f].R[:] = [float(v) for v in c.R.ravel()]
        out[f].t[:] = [float(v) for v in c.t]
        out[f].fx, out[f].fy, out[f].cx, out[f].cy, out[f].aspect_ratio, out[f].unproject_sign = c.fx, c.fy, c.cx, c.cy, c.aspect, c.sign
    return out


class _Problem:
    """pc_refine_problem of a case, or of ONE of its edges (the same arrays with n_edges = 1)"""

    def __init__(self, env, case, edge=None):
        self.L, self.ctx, meshes = env
        self.case = case
        if edge is None:
            a = dict(edge_src=case.edge_src, edge_tgt=case.edge_tgt, edge_offset=case.edge_offset, res_src_kp=case.res_src_kp,
                     res_tgt_xy=case.res_tgt_xy, edge_weight=case.edge_weight)
        else:
            sl = slice(case.edge_offset[edge], case.edge_offset[edge + 1])
            a = dict(edge_src=case.edge_src[edge:edge + 1], edge_tgt=case.edge_tgt[edge:edge + 1],
                     edge_offset=np.array([0, sl.stop - sl.start], np.int32), res_src_kp=case.res_src_kp[sl], res_tgt_xy=case.res_tgt_xy[sl],
                     edge_weight=case.edge_weight[edge:edge + 1])
        a.update(kp_offset=case.kp_offset, kp_xy=case.kp_xy)
        want = dict(kp_offset=np.int32, kp_xy=np.float32, edge_src=np.int32, edge_tgt=np.int32, edge_offset=np.int32, res_src_kp=np.uint32,
                    res_tgt_xy=np.float32, edge_weight=np.float32)
        self.arrays = {k: np.ascontiguousarray(v, want[k]) for k, v in a.items()}
        self.n_edges = len(self.arrays["edge_src"])
        d = RefineDesc()
        d.n_frames, d.n_edges = case.n_frames, self.n_edges
        for k, v in self.arrays.items():
            setattr(d, k, _p(v))
        d.model_matrix[:] = [float(v) for v in case.geom.model.ravel()]
        d.model_matrix_inv[:] = [float(v) for v in case.geom.model_inv.ravel()]
        d.block_len, d.optimize_focal_length, d.optimize_principal_point = case.B, int(case.opt_f), int(case.opt_pp)
        self.h = VP()
        assert self.L.pc_refine_problem_create(self.ctx._h, meshes[case.mesh], C.byref(d), C.byref(self.h)) == 0, self.L.pc_last_error()

    def cost(self, cams):
        out = C.c_double(np.nan)
        assert self.L.pc_refine_total_cost(self.ctx._h, self.h, _abi_cameras(cams), self.case.loss, self.case.scale, C.byref(out)) == 0
        return out.value

    def normal_equations(self, cams):
        blocks = np.full((self.n_edges, rr.n_packed(self.case.B)), np.nan)
        valid = np.full(self.n_edges, -1, np.int32)
        assert self.L.pc_refine_normal_equations(self.ctx._h, self.h, _abi_cameras(cams), self.case.loss, self.case.scale, _p(blocks), _p(valid)) == 0
        return blocks, valid

    def close(self):
        self.L.pc_refine_problem_destroy(self.h)


def _hold(name, what, key, got, want, A, r):
    """every value within BOUND_FACTOR * r * 2^-24 * A of the float64 value, exactly 0 where A is 0"""
    got, want, A = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(want), np.atleast_1d(A)
    bound = tr.BOUND_FACTOR * r * tr.EPS24 * A
    err = np.abs(got - want)
    live = A > 0
    if live.any():
        ratio = float((err[live] / bound[live]).max())
        WORST[key] = max(WORST[key], ratio) if np.isfinite(ratio) else np.inf
        print(f"{name}: {what}: worst |gpu - f64| / bound = {ratio:.4f}")
    assert np.all(got[~live] == 0.0), (name, what, "a value nothing was added to is not exactly zero")
    assert np.all(err <= bound), (name, what, np.argwhere(~(err <= bound))[:8].tolist(), float((err / np.where(live, bound, 1)).max()))


def _check_neq(name, what, got, ref, B, rho):
    blocks, valid = got
    nt = (2 * B) * (2 * B + 1) // 2
    assert np.array_equal(valid, ref.valid), (name, what, valid.tolist(), ref.valid.tolist())
    _hold(name, what + " triangle", "triangle", blocks[:, :nt], ref.packed[:, :nt], ref.A[:, :nt], rho[0])
    _hold(name, what + " gradient", "gradient", blocks[:, nt:], ref.packed[:, nt:], ref.A[:, nt:], rho[1])


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _run_case(env, rho, name):
    """the sweeps the case names, each against the restatement stepping the same cache; then the last cost sweep again, twice:
    now every triangle comes from the cache, the value is held to the same bound and the two calls give the same bits"""
    case, sel, r64, _ = rr.reference(name)
    prob = _Problem(env, case)
    try:
        for k, ((kind, cams), ref) in enumerate(zip(case.sweeps, r64)):
            what = f"sweep {k} ({case.order[k]})"
            if kind == "cost":
                _hold(name, what + " total cost", "total cost", prob.cost(cams), ref.total, ref.A_cost.sum(), rho[2])
            else:
                got = prob.normal_equations(cams)
                _check_neq(name, what, got, ref, case.B, rho)
                again = prob.normal_equations(cams)
                assert np.array_equal(_bits(got[0]), _bits(again[0])) and np.array_equal(got[1], again[1])
        last = max(k for k, (kind, _) in enumerate(case.sweeps) if kind == "cost")
        warm = [prob.cost(case.sweeps[last][1]) for _ in range(2)]
        _hold(name, "warm cache total cost", "total cost", warm[0], r64[last].total, r64[last].A_cost.sum(), rho[2])
        assert _bits(warm[0]) == _bits(warm[1])
    finally:
        prob.close()
    return case, sel, r64


@pytest.mark.parametrize("name", [pytest.param(n, id=n) for n in SPECS if n.endswith(("-opengl", "-opencv"))])
def test_model_matrix_convention_aspect_loss_and_flags(env, rho, name):
    case, _, r64 = _run_case(env, rho, name)
    assert r64[1].valid.min() > 100 and (r64[1].valid < np.diff(case.edge_offset)).all()      # every edge: valid and invalid residuals


@pytest.mark.parametrize("name", ["sizes-b6", "sizes-b9"])
def test_edge_sizes_around_the_wave_width_and_the_strides(env, rho, name):
    """edges of 0, 1, 2, 63 .. 1025 residuals in one problem (three and more trips of every kernel's lanes, waves partly idle; one
    more edge carries the weight 0),
    then every edge alone: pc_refine_total_cost returns only the total, a problem of one edge makes it the edge's cost"""
    case, _, r64 = _run_case(env, rho, name)
    assert tuple(np.diff(case.edge_offset)) == rr.SIZES_CASE_EDGES
    ref = r64[0]
    cams = case.sweeps[0][1]
    for e, size in enumerate(rr.SIZES_CASE_EDGES):
        prob = _Problem(env, case, edge=e)
        try:
            cold, warm, warm2 = prob.cost(cams), prob.cost(cams), prob.cost(cams)
            blocks, valid = prob.normal_equations(cams)
        finally:
            prob.close()
        _hold(name, f"edge of {size} alone, cost", "edge cost", cold, np.float64(ref.cost[e]), ref.A_cost[e], rho[2])
        _hold(name, f"edge of {size} alone, cost from the cache", "edge cost", warm, np.float64(ref.cost[e]), ref.A_cost[e], rho[2])
        assert _bits(warm) == _bits(warm2)
        one = copy.copy(r64[1])
        one.valid, one.packed, one.A = r64[1].valid[e:e + 1], r64[1].packed[e:e + 1], r64[1].A[e:e + 1]
        _check_neq(name, f"edge of {size} alone", (blocks, valid), one, case.B, rho)


def test_a_target_camera_that_looks_away(env, rho):
    case, _, r64 = _run_case(env, rho, "target-turned-away")
    away = (case.edge_tgt == 3) | (case.edge_src == 3)
    assert away.any() and not r64[1].valid[away].any() and not r64[1].A[away].any() and not r64[0].A_cost[away].any()


def test_the_triangle_cache_across_sweeps(env, rho):
    """cost at cameras A, cost at B (two thirds of the rays leave their cached triangle, the others keep it), normal equations at B"""
    _run_case(env, rho, "cache-across-sweeps")


def test_normal_equations_before_any_cost_sweep(env, rho):
    """nothing is cached: every block exactly zero, edge_valid 0; after a cost sweep the same call is held to the bound"""
    case, _, r64 = _run_case(env, rho, "normal-equations-first")
    assert not r64[0].A.any() and not r64[0].valid.any() and r64[2].valid.min() > 100


def test_a_cached_triangle_is_kept_although_a_nearer_one_covers_it(env, rho):
    """refiner.cc:323-331: at B every ray passes through the front triangle first and still hits the cached back triangle"""
    case, sel, _ = _run_case(env, rho, "cached-triangle-kept")
    assert (sel.closest[1] == 1).all() and (sel.used[1] == 0).all()


# ---- the host assembly of csrc/host/trajectory_refiner.cc, through polychase_core ----------------------------------------------
def test_the_assembled_system_of_polychase_core(rho, tmp_path):
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core as core
    import pnp_oracle as po
    import refine_scene as S
    name = "core-rot_scale"
    base = rr.reference(name)[0]
    assert base.matrix == "rot_scale" and base.aspect == 0.8 and base.opt_f and base.opt_pp and base.n_frames >= 5 and base.on_mesh.all()
    first = 1
    kps = {first + f: base.kp_xy[base.kp_offset[f]:base.kp_offset[f + 1]] for f in range(base.n_frames)}
    flows = {first + f: [] for f in range(base.n_frames)}
    for e in range(len(base.edge_src)):
        sl = slice(base.edge_offset[e], base.edge_offset[e + 1])
        flows[first + int(base.edge_src[e])].append((first + int(base.edge_tgt[e]), base.res_src_kp[sl], base.res_tgt_xy[sl]))
    path = str(tmp_path / "flow.db")
    S.write_database(core, path, kps, flows)
    cams = [po.Camera(fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy, aspect_ratio=c.aspect, width=960.0, height=540.0, opencv=c.sign > 0,
                      q=po.R_to_quat(c.R), t=c.t) for c in base.sweeps[0][1]]
    traj = S.to_core_trajectory(core, cams, first)
    # the restatement at the cameras the host hands to the kernel: its own float32 rotation matrix of the float32 quaternion
    host_cams = []
    for f, c in enumerate(base.sweeps[0][1]):
        st = traj.get(first + f)
        Rt = np.asarray(st.pose._Rt4x4(), np.float64)
        k = st.intrinsics
        cam = rr.make_camera(Rt[:3, :3], Rt[:3, 3], k.fy, k.aspect_ratio, k.cx, k.cy, c.sign > 0)
        assert cam.fx == float(np.float32(k.fx)) and np.abs(cam.R - c.R).max() < 1e-6
        host_cams.append(cam)
    case = copy.copy(base)
    case.sweeps = [(kind, host_cams) for kind, _ in base.sweeps]
    sel = rr.select_triangles(np.float64, case.geom, case.sweeps, case.kp_offset, case.kp_xy)
    assert sel.margin.min() >= 0.99 * rr.MARGIN and sel.gap.min() > 0 and np.array_equal(sel.used[0], rr.reference(name)[1].used[0])
    r64 = rr.evaluate(np.float64, case, sel)
    bo = core.BundleOptions()
    bo.loss_type, bo.loss_scale = core.LossType.Huber, case.scale
    mesh = core.AcceleratedMesh(case.geom.verts, case.geom.tris)
    got = core._refinement_system(path, traj, case.geom.model.astype(np.float32), mesh, True, True, bo)
    assert got["num_keypoints"] == len(case.kp_xy)                 # the bounding-box filter kept every keypoint
    assert got["num_edges"] == len(case.edge_src) and got["num_residuals"] == len(case.res_src_kp) and got["block_length"] == 9
    JtJ, Jtr = rr.scatter(case, r64[1].packed)
    nt = 18 * 19 // 2
    bound = np.concatenate([np.full((len(case.edge_src), nt), rho[0]), np.full((len(case.edge_src), 18), rho[1])], 1) * tr.BOUND_FACTOR * tr.EPS24 * r64[1].A
    bJ, br = rr.scatter(case, bound)                                # an assembled entry: the sum of its edges' bounds
    eJ, er = np.abs(np.asarray(got["JtJ"], np.float64) - JtJ), np.abs(np.asarray(got["Jtr"], np.float64) - Jtr)
    for key, err, b, g in (("assembled JtJ", eJ, bJ, got["JtJ"]), ("assembled Jtr", er, br, got["Jtr"])):
        live = b > 0
        WORST[key] = max(WORST[key], float((err[live] / b[live]).max()))
        print(f"{name}: {key}: worst |gpu - f64| / bound = {WORST[key]:.4f}, {int(live.sum())} of {live.size} entries live")
        assert np.all(np.asarray(g)[~live] == 0.0) and np.all(err <= b), (key, np.argwhere(err > b)[:8].tolist())
    assert np.array_equal(got["JtJ"], np.asarray(got["JtJ"]).T)
    fixed = np.r_[0:9, 9 * (case.n_frames - 1):9 * case.n_frames]
    assert not np.asarray(got["JtJ"])[fixed].any() and not np.asarray(got["Jtr"])[fixed].any() and np.asarray(got["Jtr"])[9:-9].all()
    cost_bound = tr.BOUND_FACTOR * rho[2] * tr.EPS24 * r64[0].A_cost.sum()
    assert abs(float(got["cost"]) - r64[0].total) <= cost_bound
    print("worst |gpu - float64| / bound:", {k: round(v, 4) for k, v in WORST.items() if k.startswith("assembled")})
