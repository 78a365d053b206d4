"""GPU: the PnP sums at the C ABI -- pc_pnp_normal_equations_cost, pc_pnp_normal_equations, pc_pnp_total_cost -- against the
float64 restatement of tests/tracker_ref.py, entry by entry.  The LM tests only see these sums through the pose a run ends at,
and Levenberg-Marquardt gets there with any descent direction; here every one of the 45 + 9 + 1 + 1 values is held to
    |gpu - float64| <= 4 * rho * 2^-24 * sum_i |term_i|
with rho the worst noise of the float32 restatement over this file's cases (measured in tests/test_tracker_ref_cpu.py,
recorded in profiles/tracker_pnp_sum_noise.txt).  Named cases: both conventions x aspect ratios x losses x intrinsics flags,
weights, points behind the camera, sizes across the wavefront / block / grid-stride edges."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from polychase_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_oracle as po  # noqa: E402
import tracker_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
VP = C.c_void_p
SPECS = tr.pnp_case_specs()
WORST = {"jtj": 0.0, "jtr": 0.0, "cost": 0.0}          # worst observed |gpu - float64| / bound, printed at the end


class PnPParams(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("aspect_ratio", C.c_float), ("convention_opencv", C.c_int), ("optimize_focal_length", C.c_int),
                ("optimize_principal_point", C.c_int), ("loss_type", C.c_int), ("loss_scale", C.c_float)]


def _p(a):
    return None if a is None else a.ctypes.data_as(VP)


@pytest.fixture(scope="module")
def env():
    L = hip.load()
    ctx = hip.Context(0)
    L.pc_pnp_problem_create.argtypes = [VP, VP, VP, VP, C.c_int, C.POINTER(VP)]
    L.pc_pnp_problem_destroy.argtypes = [VP]
    L.pc_pnp_normal_equations.argtypes = [VP, VP, C.POINTER(PnPParams), VP, VP, C.POINTER(C.c_int)]
    L.pc_pnp_normal_equations_cost.argtypes = [VP, VP, C.POINTER(PnPParams), VP, VP, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.pc_pnp_total_cost.argtypes = [VP, VP, C.POINTER(PnPParams), C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    yield L, ctx
    ctx.close()
    print("\nworst |gpu - float64| / bound:", {k: round(v, 4) for k, v in WORST.items()})


@pytest.fixture(scope="module")
def rho():
    return tr.pnp_rho_worst()


def _abi_params(p):
    q = PnPParams()
    q.R[:] = [float(v) for v in p.R.ravel()]
    q.t[:] = [float(v) for v in p.t]
    q.fx, q.fy, q.cx, q.cy, q.aspect_ratio = p.fx, p.fy, p.cx, p.cy, p.aspect_ratio
    q.convention_opencv, q.optimize_focal_length, q.optimize_principal_point = int(p.opencv), int(p.opt_f), int(p.opt_pp)
    q.loss_type, q.loss_scale = p.loss, p.scale
    return q


def _evaluate(env, c):
    """the three entry points on one problem; the header's promises between them are checked on the way:
    cost of _normal_equations_cost == pc_pnp_total_cost, pc_pnp_normal_equations == the first 54 values, the same call
    twice == the same bits"""
    L, ctx = env
    prob = VP()
    assert L.pc_pnp_problem_create(ctx._h, _p(c.X), _p(c.x), _p(c.w), c.n, C.byref(prob)) == 0, L.pc_last_error()
    q = _abi_params(c.params)
    out = []
    for _ in range(2):
        jtj, jtr = np.full(45, np.nan, np.float32), np.full(9, np.nan, np.float32)
        valid, cost = C.c_int(-1), C.c_float(math.nan)
        assert L.pc_pnp_normal_equations_cost(ctx._h, prob, C.byref(q), _p(jtj), _p(jtr), C.byref(valid), C.byref(cost)) == 0
        out.append((jtj, jtr, valid.value, np.float32(cost.value)))
    jtj2, jtr2, valid2 = np.full(45, np.nan, np.float32), np.full(9, np.nan, np.float32), C.c_int(-1)
    assert L.pc_pnp_normal_equations(ctx._h, prob, C.byref(q), _p(jtj2), _p(jtr2), C.byref(valid2)) == 0
    cost3, valid3, inliers = C.c_float(math.nan), C.c_int(-1), C.c_int(-1)
    assert L.pc_pnp_total_cost(ctx._h, prob, C.byref(q), tr.PNP_MAX_INLIER_ERROR_SQ, C.byref(cost3), C.byref(valid3), C.byref(inliers)) == 0
    L.pc_pnp_problem_destroy(prob)
    (jtj, jtr, valid, cost), again = out
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)   # noqa: E731
    assert np.array_equal(bits(jtj), bits(again[0])) and np.array_equal(bits(jtr), bits(again[1]))
    assert valid == again[2] and bits(cost) == bits(again[3])
    assert np.array_equal(bits(jtj), bits(jtj2)) and np.array_equal(bits(jtr), bits(jtr2)) and valid == valid2.value
    assert bits(cost) == bits(np.float32(cost3.value)) and valid == valid3.value
    return jtj, jtr, valid, cost, inliers.value


def _check(name, got, rho, cost_is_inf=False):
    c, t64, s64, _ = tr.pnp_reference(name)
    jtj, jtr, valid, cost, inliers = got
    assert valid == s64[2]
    for key, g, want, A, r in (("jtj", jtj, s64[0], t64.A_jtj, rho[0]), ("jtr", jtr, s64[1], t64.A_jtr, rho[1])):
        bound = tr.BOUND_FACTOR * r * tr.EPS24 * A
        err = np.abs(g.astype(np.float64) - want)
        live = A > 0
        if live.any():
            ratio = float((err[live] / bound[live]).max())
            WORST[key] = max(WORST[key], ratio)
            print(f"{name}: {key} worst |gpu - f64| / bound = {ratio:.4f}")
        assert np.all(g[~live] == 0)                                  # nothing was added: exactly zero
        assert np.all(err <= bound), (name, key, np.nonzero(err > bound)[0], (err / np.where(live, bound, 1)).max())
    # a flag that is off leaves its rows and columns exactly zero, not merely small
    off = ([6] if not c.params.opt_f else []) + ([7, 8] if not c.params.opt_pp else [])
    for k, (a, b) in enumerate(tr.TRIL):
        if a in off or b in off:
            assert jtj[k] == 0.0
    assert np.all(jtr[off] == 0.0)
    if cost_is_inf:
        assert cost == np.inf and s64[3] == np.inf
    else:
        bound = tr.BOUND_FACTOR * rho[2] * tr.EPS24 * t64.A_cost
        err = abs(float(cost) - s64[3])
        if bound > 0:
            WORST["cost"] = max(WORST["cost"], err / bound)
            print(f"{name}: cost worst |gpu - f64| / bound = {err / bound:.4f}")
        assert err <= bound, (name, float(cost), s64[3], bound)
    # inliers: the float64 count, give or take the points whose r^2 float32 cannot place against the threshold
    thr = tr.PNP_MAX_INLIER_ERROR_SQ
    near = int((np.abs(t64.r2 - thr) <= tr.BOUND_FACTOR * t64.r2_noise).sum())
    want_inliers = int((t64.r2 < thr).sum())
    print(f"{name}: inliers {inliers} float64 {want_inliers} undecidable {near}")
    assert near <= 2
    assert abs(inliers - want_inliers) <= near
    return c, t64, s64


@pytest.mark.parametrize("name", [pytest.param(n, id=n) for n in SPECS if n.startswith(("opengl-", "opencv-"))])
def test_convention_aspect_loss_and_flags(env, rho, name):
    c = tr.pnp_reference(name)[0]
    _, t64, _ = _check(name, _evaluate(env, c), rho)
    assert not t64.behind.any()


def test_weights(env, rho):
    null = _evaluate(env, tr.pnp_reference("weights-null")[0])
    ones = _evaluate(env, tr.pnp_reference("weights-ones")[0])
    _check("weights-null", null, rho)
    # a weight of one is what no weights means: the same bits
    for a, b in zip(null, ones):
        assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    c, t64, _ = _check("weights-mixed", _evaluate(env, tr.pnp_reference("weights-mixed")[0]), rho)
    assert 0 < t64.valid.sum() < c.n and set(np.unique(c.w)) == {0.0, 0.25, 1.0, 3.0}
    jtj, jtr, valid, cost, inliers = _evaluate(env, tr.pnp_reference("weights-zero")[0])
    assert not jtj.any() and not jtr.any() and valid == 0 and cost == 0.0
    assert inliers > 0                              # the inlier count of SolvePnPIterative does not look at the weights
    _check("weights-zero", (jtj, jtr, valid, cost, inliers), rho)


@pytest.mark.parametrize("name", [pytest.param(n, id=n) for n in SPECS if n.startswith("behind-")])
def test_points_behind_the_camera(env, rho, name):
    """a point behind the camera still counts as valid and still enters the normal equations (EvaluateWithJacobian returns
    true); the cost is +inf under every loss; it is no inlier; with weight 0 on exactly those points the cost is finite"""
    c = tr.pnp_reference(name)[0]
    zero_weighted = c.w is not None
    got = _evaluate(env, c)
    _, t64, _ = _check(name, got, rho, cost_is_inf=not zero_weighted)
    n_behind = int(c.is_behind.sum())
    assert np.array_equal(t64.behind, c.is_behind) and 0.02 * c.n < n_behind < 0.09 * c.n
    assert got[2] == (c.n - n_behind if zero_weighted else c.n)
    assert got[4] <= c.n - n_behind
    if zero_weighted:
        assert np.isfinite(got[3]) and got[3] > 0


@pytest.mark.parametrize("n", tr.PNP_SIZES)
def test_sizes_across_wavefront_block_and_grid_edges(env, rho, n):
    """1 / 5 / 65 / 512 blocks in the second stage; 131073 is the first size at which a lane takes a second correspondence"""
    name = f"size-{n}"
    _check(name, _evaluate(env, tr.pnp_reference(name)[0]), rho)


# ---- solver level: OpenCV convention, aspect_ratio != 1, both intrinsics flags ----------------------------------------------
def _angle(Ra, Rb):
    return math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1) / 2)))


def test_solver_with_an_opencv_camera_and_free_intrinsics(monkeypatch):
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core as core
    W, H, F, aspect = tr.PNP_W, tr.PNP_H, tr.PNP_F, 1.07
    rng = np.random.default_rng(23)
    Xw = rng.uniform(-2, 2, (1500, 3))
    R = tr._rot([0.2, 1.0, 0.1], 0.3)
    t = np.array([0.1, -0.15, 7.0])
    truth = po.Camera(fx=F * aspect, fy=F, cx=W / 2 + 6, cy=H / 2 - 4, aspect_ratio=aspect, width=W, height=H, opencv=True,
                      q=po.R_to_quat(R), t=t)
    x, Z = truth.project_world(Xw)
    assert (Z[:, 2] > 0).all()
    X32 = Xw.astype(np.float32)
    fy0 = F * 0.97
    k0 = core.CameraIntrinsics(fx=fy0 * aspect, fy=fy0, cx=W / 2, cy=H / 2, aspect_ratio=aspect, width=W, height=H,
                               convention=core.CameraConvention.OpenCV)
    init = core.CameraState(k0, core.Pose())
    R0, t0 = tr._rot([0.3, 1, 0.2], 0.01) @ R, t + [0.03, -0.02, 0.05]
    p = core.Pose()
    p.q, p.t = po.R_to_quat(R0).astype(np.float32), t0.astype(np.float32)
    init.pose = p
    bo = core.BundleOptions()
    noisy = x + rng.normal(0, 0.4, x.shape)
    noisy[::37] += rng.uniform(-80, 80, noisy[::37].shape)
    for kind, x32 in (("noise-free", x.astype(np.float32)), ("noisy", noisy.astype(np.float32))):
        args = (X32, x32, init, bo, 12.0, True, True)
        monkeypatch.delenv("POLYCHASE_PNP_HOST_LM", raising=False)
        dev = core._solve_pnp_iterative(*args)
        o_init = po.Camera(fx=float(np.float32(fy0 * aspect)), fy=float(np.float32(fy0)), cx=W / 2, cy=H / 2, aspect_ratio=float(np.float32(aspect)),
                           width=W, height=H, opencv=True, q=po.R_to_quat(R0).astype(np.float32).astype(float), t=t0.astype(np.float32).astype(float))
        ocam, _ = po.solve_pnp(X32, x32, o_init, kind="huber", scale=bo.loss_scale, opt_f=True, opt_pp=True)
        Rg, tg = po.quat_to_R(np.array(dev.camera.pose.q, float)), np.array(dev.camera.pose.t, float)
        k = dev.camera.intrinsics
        print(kind, "solver: angle to oracle", _angle(Rg, ocam.R()), "dt/|t|", np.linalg.norm(tg - ocam.t) / np.linalg.norm(ocam.t),
              "fy, cx, cy off the truth", k.fy - F, k.cx - truth.cx, k.cy - truth.cy, "fx - fy * aspect", k.fx - k.fy * aspect)
        assert _angle(Rg, ocam.R()) <= 1e-4
        assert np.linalg.norm(tg - ocam.t) <= 1e-4 * np.linalg.norm(ocam.t)
        if kind == "noise-free":
            assert abs(k.fy - F) < 0.5 and abs(k.cx - truth.cx) < 0.5 and abs(k.cy - truth.cy) < 0.5
        assert abs(k.fx - k.fy * aspect) <= 1e-3
        # the host-driven loop: the tolerances of test_device_resident_lm_equals_the_host_driven_loop
        monkeypatch.setenv("POLYCHASE_PNP_HOST_LM", "1")
        host = core._solve_pnp_iterative(*args)
        sd, sh = dev.bundle_stats, host.bundle_stats
        assert sd.iterations == sh.iterations and sd.invalid_steps == sh.invalid_steps
        assert sd.initial_cost == sh.initial_cost
        assert abs(sd.cost - sh.cost) <= 1e-5 * abs(sh.cost)
        assert np.allclose(np.array(dev.camera.pose.q), np.array(host.camera.pose.q), atol=2e-6)
        assert np.allclose(np.array(dev.camera.pose.t), np.array(host.camera.pose.t), atol=2e-5)
        assert abs(dev.camera.intrinsics.fy - host.camera.intrinsics.fy) <= 1e-4 * abs(host.camera.intrinsics.fy)
        assert dev.inlier_ratio == host.inlier_ratio
