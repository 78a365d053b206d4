"""Plain numpy restatements of the tracking kernels' arithmetic, runnable in float64 (the reference) and in float32 (the
noise model the GPU bounds are taken from), plus the fixed scenes the tracker edge-case tests share.  No GPU.

  pnp_terms    per-correspondence terms of the 45 + 9 + 1 + 1 sums of the PnP sweep
               (PnPProblem::EvaluateWithJacobian, CameraIntrinsics::ProjectWithJac / IsBehind, the robust losses and the
               weight handling of LevMarqDenseSolver::BuildNormalEquations / TotalCost)
  mt_closest   closest hit by Moeller-Trumbore with the reference's 1e-10 determinant gate, lowest index among equal t,
               with the float64 margins of the decision

How a bound is made (tests/test_tracker_ref_cpu.py measures, the GPU tests apply):
  rho = max_k |sum32_k - sum64_k| / (2^-24 * A_k),  A_k = sum_i |term_i|   over every PnP case below, per kind of sum;
  a GPU sum may differ from the float64 sum by 4 * rho_worst * 2^-24 * A_k.  The factor 4 is for the kernel's different,
  equally valid operation and summation order.  The ray-cast gates are 4 x the worst float32-vs-float64 difference of the
  restatement over the scenes below.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

EPS24 = 2.0 ** -24
BOUND_FACTOR = 4.0
LOSSES = ("trivial", "huber", "cauchy")
MUTANTS = ("no_aspect", "behind_sign", "no_weight", "huber_r2", "d02_sign")
TRIL = [(a, b) for a in range(9) for b in range(a + 1)]          # packed row-major lower triangle


# ---------------------------------------------------------------------------------------------------------------------
# PnP
# ---------------------------------------------------------------------------------------------------------------------
def make_params(R, t, fx, fy, cx, cy, aspect_ratio, opencv, opt_f, opt_pp, loss, scale):
    """every float is rounded to float32 once: the float64 and the float32 run (and the GPU) start from the same numbers"""
    f = lambda v: float(np.float32(v))   # noqa: E731
    return SimpleNamespace(R=np.asarray(R, np.float32).astype(np.float64).reshape(3, 3), t=np.asarray(t, np.float32).astype(np.float64),
                           fx=f(fx), fy=f(fy), cx=f(cx), cy=f(cy), aspect_ratio=f(aspect_ratio), opencv=bool(opencv),
                           opt_f=bool(opt_f), opt_pp=bool(opt_pp), loss=LOSSES.index(loss) if isinstance(loss, str) else int(loss),
                           scale=f(scale))


def _loss(dtype, kind, scale, r2, mutant=None):
    """(weight, value) of the robust loss at r2; r2 may be +inf"""
    one = dtype(1.0)
    if kind == 0:
        return np.ones_like(r2), r2
    if kind == 1:
        r = np.sqrt(r2)
        inside = r2 <= scale * scale
        denom = r2 if mutant == "huber_r2" else r
        wgt = np.where(inside, one, scale / np.where(inside, one, denom))
        return wgt, np.where(inside, r2, scale * (dtype(2.0) * r - scale))
    sq = scale * scale
    inv_sq = one / sq
    return np.maximum(dtype(np.finfo(np.float32).tiny), one / (one + r2 * inv_sq)), sq * np.log1p(r2 * inv_sq)


def pnp_terms(dtype, params, X, x, w=None, mutant=None):
    """Per-correspondence terms, computed in `dtype`.  Returns a namespace:
      jtj [n, 45], jtr [n, 9], cost [n]   terms of the sums (zero rows where weight == 0)
      valid [n] bool                      weight != 0 (a point behind the camera still counts: EvaluateWithJacobian is true)
      behind [n] bool, r2 [n]             r2 = +inf behind the camera (what TotalCost and the inlier count see)
      A_jtj [45], A_jtr [9], A_cost       sums of the absolute terms
      J [n, 2, 9], r [n, 2]               the Jacobian and the residual themselves
    `mutant` plants one named error (tests/test_tracker_ref_cpu.py: the bound has to notice it)."""
    dtype = np.dtype(dtype).type
    X, x = np.asarray(X).astype(dtype), np.asarray(x).astype(dtype)
    n = len(X)
    weight = np.ones(n, dtype) if w is None else np.asarray(w).astype(dtype)
    R, t = params.R.astype(dtype), params.t.astype(dtype)
    fx, fy, cx, cy, ar, scale = (dtype(v) for v in (params.fx, params.fy, params.cx, params.cy, params.aspect_ratio, params.scale))
    zero, one = np.zeros(n, dtype), np.ones(n, dtype)
    with np.errstate(all="ignore"):
        # RtZ = R Z + t
        a = [R[k, 0] * X[:, 0] + R[k, 1] * X[:, 1] + R[k, 2] * X[:, 2] + t[k] for k in range(3)]
        ax, ay, az = a
        rx, ry = fx * ax / az + cx - x[:, 0], fy * ay / az + cy - x[:, 1]
        d00, d02 = fx / az, -fx * ax / (az * az)
        d11, d12 = fy / az, -fy * ay / (az * az)
        if mutant == "d02_sign":
            d02 = -d02
        # dRtZ_dR = R * Skew(-Z)
        M = [[-R[k, 1] * X[:, 2] + R[k, 2] * X[:, 1], R[k, 0] * X[:, 2] - R[k, 2] * X[:, 0], -R[k, 0] * X[:, 1] + R[k, 1] * X[:, 0]]
             for k in range(3)]
        J0 = [d00 * M[0][c] + d02 * M[2][c] for c in range(3)] + [d00, zero, d02]
        J1 = [d11 * M[1][c] + d12 * M[2][c] for c in range(3)] + [zero, d11, d12]
        focal0 = ax / az if mutant == "no_aspect" else ar * ax / az
        J0 += [focal0 if params.opt_f else zero, one if params.opt_pp else zero, zero]
        J1 += [ay / az if params.opt_f else zero, zero, one if params.opt_pp else zero]
        r2 = rx * rx + ry * ry
        opencv = params.opencv != (mutant == "behind_sign")
        behind = (az < 0) if opencv else (az > 0)
        lw, _ = _loss(dtype, params.loss, scale, r2, mutant)
        r2c = np.where(behind, dtype(np.inf), r2)
        _, lv = _loss(dtype, params.loss, scale, r2c)
        valid = weight != 0
        tw = (lw if mutant == "no_weight" else weight * lw)
        tw = np.where(valid, tw, dtype(0))
        jtj = np.stack([tw * (J0[p] * J0[q] + J1[p] * J1[q]) for p, q in TRIL], 1)
        jtr = np.stack([J0[p] * (tw * rx) + J1[p] * (tw * ry) for p in range(9)], 1)
        cost = np.where(valid, (one if mutant == "no_weight" else weight) * lv, dtype(0))
        A_jtj = np.stack([tw * (np.abs(J0[p] * J0[q]) + np.abs(J1[p] * J1[q])) for p, q in TRIL], 1).sum(0)
        A_jtr = np.stack([np.abs(J0[p] * (tw * rx)) + np.abs(J1[p] * (tw * ry)) for p in range(9)], 1).sum(0)
        jtj[~valid], jtr[~valid] = 0, 0
        A_cost = np.abs(cost).sum()
    return SimpleNamespace(jtj=jtj, jtr=jtr, cost=cost, valid=valid, behind=behind, r2=r2c, A_jtj=A_jtj, A_jtr=A_jtr, A_cost=A_cost,
                           J=np.stack([np.stack(J0, 1), np.stack(J1, 1)], 1), r=np.stack([rx, ry], 1))


def pnp_sums(terms):
    """(jtj45, jtr9, valid, cost) summed in the terms' own dtype"""
    with np.errstate(all="ignore"):
        return terms.jtj.sum(0), terms.jtr.sum(0), int(terms.valid.sum()), terms.cost.sum()


def pnp_rho(s32, s64, t64):
    """(rho_jtj, rho_jtr, rho_cost) of one case; an entry whose absolute sum is 0 has to be exactly 0 in both"""
    out = []
    for got, want, A in ((s32[0], s64[0], t64.A_jtj), (s32[1], s64[1], t64.A_jtr), (s32[3], s64[3], t64.A_cost)):
        got, want, A = np.atleast_1d(np.float64(got)), np.atleast_1d(want), np.atleast_1d(A)
        live = (A > 0) & np.isfinite(A)
        assert np.all(got[A == 0] == 0) and np.all(want[A == 0] == 0)
        out.append(float((np.abs(got[live] - want[live]) / (EPS24 * A[live])).max()) if live.any() else 0.0)
    return tuple(out)


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K


PNP_W, PNP_H, PNP_F = 960.0, 540.0, 1100.0
PNP_MAX_INLIER_ERROR_SQ = 225.0


def pnp_case(name, n=2000, opencv=False, aspect=1.0, loss="cauchy", opt_f=True, opt_pp=True, weights=None, behind=False, seed=0):
    """One named scene: points in [-2, 2]^3, the camera 3.6-12 units away (3.6: the cube's corners stay in front) and
    rotated up to 0.6 rad, observations = projection + 2 px noise, every seventh an outlier of 30-60 px (so that next to
    nobody sits at the inlier threshold of 15 px, whatever n is); evaluated at a pose a little off the true one.  weights: None | "ones" | "mixed" | "zero" | "zero_behind"; behind: 5 % of the points are
    mirrored to the other side of the camera."""
    rng = np.random.default_rng([seed, n, int(opencv), int(aspect * 100)])
    X = rng.uniform(-2, 2, (n, 3))
    R = _rot(rng.normal(size=3), rng.uniform(0.1, 0.6))
    dist = rng.uniform(3.6, 12.0)
    t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), dist if opencv else -dist])
    fy = PNP_F if opencv else -PNP_F
    fx, cx, cy = fy * aspect, PNP_W / 2, PNP_H / 2
    Z = X @ R.T + t
    obs = np.stack([fx * Z[:, 0] / Z[:, 2] + cx, fy * Z[:, 1] / Z[:, 2] + cy], 1) + rng.normal(0, 2.0, (n, 2))
    out = np.arange(n) % 7 == 3
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(30, 60, n)
    obs[out] += (mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))[out]
    is_behind = np.zeros(n, bool)
    if behind:
        is_behind = rng.uniform(size=n) < 0.05
        is_behind[0] = n > 1
        Zb = Z * [1, 1, -1]
        X = np.where(is_behind[:, None], (Zb - t) @ R, X)
    w = {None: None, "ones": np.ones(n), "zero": np.zeros(n), "mixed": rng.choice([0.0, 0.25, 1.0, 3.0], n),
         "zero_behind": np.where(is_behind, 0.0, 1.0)}[weights]
    Re = _rot([0.3, 1.0, 0.2], 0.0005) @ R
    te = t + [0.002, -0.002, 0.004]
    p = make_params(Re, te, fx, fy, cx, cy, aspect, opencv, opt_f, opt_pp, loss, 1.5)
    return SimpleNamespace(name=name, params=p, X=X.astype(np.float32), x=obs.astype(np.float32),
                           w=None if w is None else w.astype(np.float32), n=n, is_behind=is_behind)


PNP_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 16385, 131072, 131073, 200000)


def pnp_case_specs():
    """name -> keyword arguments of pnp_case: the fixed list of sections 2 and 3"""
    specs = {}
    for opencv in (False, True):
        conv = "opencv" if opencv else "opengl"
        for aspect in (1.0, 0.8, 1.07):
            for loss in LOSSES:
                for opt_f in (False, True):
                    for opt_pp in (False, True):
                        specs[f"{conv}-a{aspect}-{loss}-f{int(opt_f)}-pp{int(opt_pp)}"] = dict(
                            opencv=opencv, aspect=aspect, loss=loss, opt_f=opt_f, opt_pp=opt_pp)
        for loss in LOSSES:
            specs[f"behind-{conv}-{loss}"] = dict(opencv=opencv, aspect=1.07, loss=loss, behind=True)
        specs[f"behind-zero-weight-{conv}"] = dict(opencv=opencv, aspect=0.8, loss="huber", behind=True, weights="zero_behind")
    for wk in ("ones", "mixed", "zero"):
        specs[f"weights-{wk}"] = dict(opencv=True, aspect=1.07, loss="huber", weights=wk)
    specs["weights-null"] = dict(opencv=True, aspect=1.07, loss="huber")
    for n in PNP_SIZES:
        specs[f"size-{n}"] = dict(n=n, opencv=True, aspect=1.07, loss="cauchy")
    return specs


_pnp_cache = {}


def pnp_reference(name):
    """(case, float64 terms, float64 sums, rho of the float32 restatement) of a named case, computed once per process"""
    if name not in _pnp_cache:
        c = pnp_case(name, **pnp_case_specs()[name])
        t64 = pnp_terms(np.float64, c.params, c.X, c.x, c.w)
        s64 = pnp_sums(t64)
        t32 = pnp_terms(np.float32, c.params, c.X, c.x, c.w)
        rho = pnp_rho(pnp_sums(t32), s64, t64)
        # noise of r^2 where it matters for the inlier count: around the threshold (it grows with r)
        with np.errstate(invalid="ignore"):
            dr2 = np.abs(np.where(np.isfinite(t64.r2), t32.r2.astype(np.float64) - t64.r2, 0.0))
        around = (t64.r2 > PNP_MAX_INLIER_ERROR_SQ / 2) & (t64.r2 < PNP_MAX_INLIER_ERROR_SQ * 2)
        r2_noise = float(dr2[around].max() if around.any() else dr2.max())
        # keep what the tests read; the [n, 45] arrays of the large cases are not needed again
        slim = SimpleNamespace(A_jtj=t64.A_jtj, A_jtr=t64.A_jtr, A_cost=t64.A_cost, r2=t64.r2, behind=t64.behind, valid=t64.valid,
                               r2_noise=r2_noise)
        _pnp_cache[name] = (c, slim, s64, rho)
    return _pnp_cache[name]


def pnp_rho_worst():
    """the three worst rho over the whole case list"""
    rho = np.array([pnp_reference(name)[3] for name in pnp_case_specs()])
    return tuple(float(v) for v in rho.max(0))


# ---------------------------------------------------------------------------------------------------------------------
# ray casting
# ---------------------------------------------------------------------------------------------------------------------
def mt_closest(dtype, verts, tris, origin, dirs, chunk=512):
    """Closest hit of every ray over all triangles, computed in `dtype`: Moeller-Trumbore with the 1e-10 determinant gate,
    u in [0, 1], v >= 0, u + v <= 1, t >= 0; the smallest t wins, the lowest index among equal t.
    Returns a namespace: hit, prim (-1 on a miss), u, v, t, pos (Triangle::Barycentric) and, as float64 margins of the decision,
      m_bary  smallest |min(u, v, 1 - u - v)| over the triangles the ray could reach first (the winner, and every triangle not
              behind the origin and not beyond the winner -- a near miss in front of it would change the answer as well)
      m_det   distance of the winner's |det| from the gate
      m_t     gap in t between the winner and the runner-up hit (inf if there is none)"""
    dtype = np.dtype(dtype).type
    V = np.asarray(verts).astype(dtype)
    tris = np.asarray(tris).astype(np.int64)
    o = np.asarray(origin).astype(dtype)
    D = np.asarray(dirs).astype(dtype)
    p1, p2, p3 = V[tris[:, 0]], V[tris[:, 1]], V[tris[:, 2]]
    e1, e2 = p2 - p1, p3 - p1
    s = o[None, :] - p1                                                    # [T, 3]
    q = np.stack([s[:, 1] * e1[:, 2] - s[:, 2] * e1[:, 1], s[:, 2] * e1[:, 0] - s[:, 0] * e1[:, 2],
                  s[:, 0] * e1[:, 1] - s[:, 1] * e1[:, 0]], 1)             # s x edge1
    tq = e2[:, 0] * q[:, 0] + e2[:, 1] * q[:, 1] + e2[:, 2] * q[:, 2]
    n = len(D)
    res = SimpleNamespace(hit=np.zeros(n, bool), prim=np.full(n, -1), u=np.zeros(n, dtype), v=np.zeros(n, dtype), t=np.zeros(n, dtype),
                          m_bary=np.full(n, np.inf), m_det=np.full(n, np.inf), m_t=np.full(n, np.inf))
    gate = dtype(1e-10)
    with np.errstate(all="ignore"):
        for lo in range(0, n, chunk):
            d = D[lo:lo + chunk]
            dx, dy, dz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
            cx = dy * e2[None, :, 2] - dz * e2[None, :, 1]
            cy = dz * e2[None, :, 0] - dx * e2[None, :, 2]
            cz = dx * e2[None, :, 1] - dy * e2[None, :, 0]                 # dir x edge2, [R, T]
            det = e1[None, :, 0] * cx + e1[None, :, 1] * cy + e1[None, :, 2] * cz
            live = ~((det > -gate) & (det < gate))
            inv = dtype(1.0) / np.where(live, det, dtype(1.0))
            u = inv * (s[None, :, 0] * cx + s[None, :, 1] * cy + s[None, :, 2] * cz)
            v = inv * (dx * q[None, :, 0] + dy * q[None, :, 1] + dz * q[None, :, 2])
            t = inv * tq[None, :]
            ok = live & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & ~(t < 0)
            tk = np.where(ok, t, dtype(np.inf))
            win = tk.argmin(1)                                             # first index among equal t
            rows = np.arange(len(d))
            hit = ok[rows, win]
            sl = slice(lo, lo + len(d))
            res.hit[sl] = hit
            res.prim[sl] = np.where(hit, win, -1)
            res.u[sl], res.v[sl], res.t[sl] = (np.where(hit, a[rows, win], dtype(0)) for a in (u, v, t))
            # margins (meaningful for the float64 run)
            t_win = np.where(hit, tk[rows, win], np.inf).astype(np.float64)
            edge = np.abs(np.minimum(np.minimum(u, v), dtype(1.0) - u - v)).astype(np.float64)
            reach = live & (t >= 0) & (t.astype(np.float64) <= t_win[:, None])
            res.m_bary[sl] = np.where(reach, edge, np.inf).min(1)
            res.m_det[sl] = np.where(hit, np.abs(np.abs(det[rows, win].astype(np.float64)) - 1e-10), np.inf)
            tk2 = tk.astype(np.float64).copy()
            tk2[rows, win] = np.inf
            res.m_t[sl] = np.where(hit, tk2.min(1) - t_win, np.inf)
    idx = np.maximum(res.prim, 0)
    a, b, c = V[tris[idx, 0]], V[tris[idx, 1]], V[tris[idx, 2]]
    w0 = dtype(1.0) - res.u - res.v
    res.pos = np.where(res.hit[:, None], w0[:, None] * a + res.u[:, None] * b + res.v[:, None] * c, dtype(0))
    return res


def grid_mesh(n=20, size=4.0):
    """the wavy (n x n)-cell grid tests/test_tracker_gpu.py uses"""
    xs = np.linspace(-size / 2, size / 2, n + 1)
    X, Y = np.meshgrid(xs, xs)
    Z = 0.3 * np.sin(1.3 * X) * np.cos(1.1 * Y)
    verts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.float32)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    tris = np.stack([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)], 1).reshape(-1, 3)
    return verts, tris.astype(np.uint32)


RC_W, RC_H = 960.0, 540.0


def raycast_scene_specs():
    """name -> (model matrix, opencv): the model matrices of section 4(b), each under both conventions, fx != fy"""
    Rm = _rot([0.3, -1.0, 0.5], 0.7)
    rot_scale = np.eye(4)
    rot_scale[:3, :3] = Rm @ np.diag([1.4, 0.8, 1.1])
    rot_scale[:3, 3] = [0.3, -0.2, 0.4]
    shear = np.eye(4)
    shear[0, 1], shear[1, 2], shear[0, 3] = 0.35, -0.2, 0.1
    mirror = np.diag([-1.2, 1.0, 0.9, 1.0])
    mirror[:3, 3] = [0.1, 0.2, -0.1]
    diag = np.diag([1.5, 1.5, 1.5, 1.0])
    return {f"{k}-{'opencv' if cv else 'opengl'}": (m.astype(np.float32), cv)
            for k, m in (("rot_scale", rot_scale), ("shear", shear), ("mirror", mirror), ("diagonal", diag)) for cv in (False, True)}


def raycast_scene(name, n_rays=3000):
    """mesh, model, view (float32 4x4), intrinsics and pixels of a named scene; the camera looks at the mesh from 8 units;
    some pixels lie outside the image"""
    model, opencv = raycast_scene_specs()[name]
    verts, tris = grid_mesh()
    rng = np.random.default_rng(sorted(raycast_scene_specs()).index(name) + 100)
    R = _rot([0.2, 1.0, 0.1], 0.05) @ _rot([1, 0, 0], 0.03)
    t = np.array([0.05, -0.04, -8.0])
    if opencv:                                       # the same camera seen as OpenCV: y and z of the view flip
        flip = np.diag([1.0, -1.0, -1.0])
        R, t = flip @ R, flip @ t
    view = np.eye(4, dtype=np.float32)
    view[:3, :3], view[:3, 3] = R, t
    fy = 1100.0 if opencv else -1100.0
    fx = fy * 1.07
    xy = rng.uniform([-150, -150], [RC_W + 150, RC_H + 150], (n_rays, 2)).astype(np.float32)
    return SimpleNamespace(name=name, verts=verts, tris=tris, model=model, view=view, opencv=opencv, fx=fx, fy=fy, cx=RC_W / 2,
                           cy=RC_H / 2, xy=xy)


def scene_rays(dtype, sc):
    """(origin, dirs) in object space.  float64: from the float64 inverse of view * model.  float32: the host's path --
    the product in float32, its inverse in double rounded to float32, unprojection and rotation in float32."""
    dtype = np.dtype(dtype).type
    if dtype is np.float32:
        inv = np.linalg.inv((sc.view @ sc.model).astype(np.float64)).astype(np.float32)
    else:
        inv = np.linalg.inv(sc.view.astype(np.float64) @ sc.model.astype(np.float64))
    s = dtype(1.0 if sc.opencv else -1.0)
    xy = sc.xy.astype(dtype)
    ux, uy = s * ((xy[:, 0] - dtype(sc.cx)) / dtype(sc.fx)), s * ((xy[:, 1] - dtype(sc.cy)) / dtype(sc.fy))
    uz = np.full(len(xy), s, dtype)
    m = inv[:3, :3]
    dirs = np.stack([m[k, 0] * ux + m[k, 1] * uy + m[k, 2] * uz for k in range(3)], 1)
    return inv[:3, 3].copy(), dirs


_rc_cache = {}


def raycast_reference(name):
    """(scene, float64 result, float32 result, (delta_bary, delta_t, delta_pos)) of a named scene, once per process"""
    if name not in _rc_cache:
        sc = raycast_scene(name)
        r64 = mt_closest(np.float64, sc.verts, sc.tris, *scene_rays(np.float64, sc))
        r32 = mt_closest(np.float32, sc.verts, sc.tris, *scene_rays(np.float32, sc))
        same = r64.hit & r32.hit & (r64.prim == r32.prim)
        d = lambda a, b: float(np.abs(a[same].astype(np.float64) - b[same]).max())   # noqa: E731
        _rc_cache[name] = (sc, r64, r32, (max(d(r32.u, r64.u), d(r32.v, r64.v)), d(r32.t, r64.t), d(r32.pos, r64.pos)))
    return _rc_cache[name]


def raycast_gates():
    """(gate_bary, gate_t, gate_pos) = 4 x the worst float32-vs-float64 difference over every scene"""
    deltas = np.array([raycast_reference(name)[3] for name in raycast_scene_specs()])
    return tuple(float(BOUND_FACTOR * v) for v in deltas.max(0))


def raycast_ambiguous(r64, gates):
    """rays whose float64 decision is closer to a boundary than float32 arithmetic can tell"""
    return (r64.m_bary < gates[0]) | (r64.m_t < gates[1]) | (r64.m_det < 1e-10)
