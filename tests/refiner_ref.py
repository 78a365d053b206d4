"""Plain numpy restatement of the two refiner sweeps -- the cost sweep (RefinementProblemBase::Evaluate + TotalCost) and the
normal-equation sweep (EvaluateWithJacobian + BuildNormalEquations) -- runnable in float64 (the reference) and in float32 (the
noise model the GPU bound is taken from), plus the named problems tests/test_refiner_ref_cpu.py and
tests/test_refine_edges_gpu.py share.  No GPU.

  edge_terms        one edge, every residual at once: valid, residual, loss value, weight, the 2 x 2B Jacobian, and from them the
                    packed per-edge outputs of pc_refine_normal_equations (lower triangle row-major, then the 2B gradient
                    entries, normalised by the valid count, times the edge weight), the per-edge cost, and for every output
                    value k  A_k = sum_i |term_i| / n_valid
  select_triangles  the triangle of every (sweep, keypoint), stepping the per-keypoint cache like the oracle: the cached triangle
                    first, on a miss the closest hit (tracker_ref.mt_closest), a masked closest hit counts as a miss
  case_specs        the named problems; every keypoint is constructed so that its triangle is decided with a float64 margin
                    (MARGIN) float32 cannot cross: no residual is excused from a comparison

How the bound is made (tests/test_refiner_ref_cpu.py measures and records, the GPU test applies):
  rho = max_k |v32_k - v64_k| / (2^-24 * A_k) over every named case, separately for triangle entries, gradient entries and the
  cost; a GPU value may differ from the float64 value by tracker_ref.BOUND_FACTOR * rho_worst * 2^-24 * A_k, and a value whose
  A_k is 0 has to be exactly 0.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import tracker_ref as tr

EPS24 = tr.EPS24
LOSSES = tr.LOSSES
MARGIN = 1e-3          # float64 barycentric margin of every triangle decision: ~24 x the gate in profiles/tracker_raycast_gates.txt
MUTANTS = ("no_aspect_src", "no_aspect_tgt", "focal_sign_src", "normal_not_transposed", "dir_not_through_model_inv", "pp_swapped",
           "tgt_behind_sign", "no_edge_weight", "huber_r2")


def n_packed(B):
    return (2 * B) * (2 * B + 1) // 2 + 2 * B


def tril(B):
    return [(a, b) for a in range(2 * B) for b in range(a + 1)]


def make_camera(R, t, fy, aspect, cx, cy, opencv):
    """the camera the way the kernel gets it: R (row-major 3x3), t, fx, fy, cx, cy, aspect, sign -- every number rounded to
    float32 once, kept as float64 so that the float64 and the float32 run (and the GPU) start from the same values"""
    f = lambda v: float(np.float32(v))   # noqa: E731
    return SimpleNamespace(R=np.asarray(R, np.float32).astype(np.float64).reshape(3, 3), t=np.asarray(t, np.float32).astype(np.float64),
                           fx=f(f(fy) * f(aspect)), fy=f(fy), cx=f(cx), cy=f(cy), aspect=f(aspect), sign=1.0 if opencv else -1.0)


def _cam(dtype, c):
    return (c.R.astype(dtype), c.t.astype(dtype), dtype(c.fx), dtype(c.fy), dtype(c.cx), dtype(c.cy), dtype(c.aspect), dtype(c.sign))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _center(R, t):
    """Pose::Center() = -R^T t"""
    return [-(R[0, k] * t[0] + R[1, k] * t[1] + R[2, k] * t[2]) for k in range(3)]


def _point(M, p):
    """affine 4x4 applied to a point, with the homogeneous divide of hnormalized()"""
    w = M[3, 0] * p[0] + M[3, 1] * p[1] + M[3, 2] * p[2] + M[3, 3]
    return [(M[k, 0] * p[0] + M[k, 1] * p[1] + M[k, 2] * p[2] + M[k, 3]) / w for k in range(3)]


def source_rays(dtype, geom, cs, sp, mutant=None):
    """object-space origin (3 scalars) and directions (3 columns) of the source keypoints' rays (refiner.cc:310-321)"""
    dtype = np.dtype(dtype).type
    R, t, fx, fy, cx, cy, _, s = _cam(dtype, cs)
    Mi = geom.model_inv.astype(dtype)
    sp = np.asarray(sp).astype(dtype)
    o = _point(Mi, _center(R, t))
    dc = [s * ((sp[:, 0] - cx) / fx), s * ((sp[:, 1] - cy) / fy), np.full(len(sp), s, dtype)]
    dw = [R[0, k] * dc[0] + R[1, k] * dc[1] + R[2, k] * dc[2] for k in range(3)]
    if mutant == "dir_not_through_model_inv":
        return o, dw
    return o, [Mi[k, 0] * dw[0] + Mi[k, 1] * dw[1] + Mi[k, 2] * dw[2] for k in range(3)]


def ray_triangle(dtype, o, d, p1, p2, p3):
    """Moeller-Trumbore of one triangle per ray (cpp/ray_casting.h:125-179): hit, t, and |min(u, v, 1 - u - v)|"""
    dtype = np.dtype(dtype).type
    e1, e2 = [p2[:, k] - p1[:, k] for k in range(3)], [p3[:, k] - p1[:, k] for k in range(3)]
    c = _cross(d, e2)
    det = _dot(e1, c)
    gate = dtype(1e-10)
    live = ~((det > -gate) & (det < gate))
    inv = dtype(1.0) / np.where(live, det, dtype(1.0))
    s = [o[k] - p1[:, k] for k in range(3)]
    u = inv * _dot(s, c)
    q = _cross(s, e1)
    v = inv * _dot(d, q)
    t = inv * _dot(e2, q)
    hit = live & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & ~(t < 0)
    return hit, t, np.abs(np.minimum(np.minimum(u, v), dtype(1.0) - u - v)).astype(np.float64)


def _loss(dtype, kind, scale, r2, mutant=None):
    return tr._loss(dtype, kind, scale, r2, mutant)


def edge_terms(dtype, geom, cs, ct, sp, tp, prim_cost, prim_neq, weight, loss, scale, B, opt_f, opt_pp, src_fixed, tgt_fixed, mutant=None):
    """One edge, computed entirely in `dtype`.  geom: verts, tris, model, model_inv (4x4, the numbers the kernel gets); cs / ct:
    make_camera; sp / tp [m, 2]: source keypoints and tracked target positions; prim_cost / prim_neq [m]: the triangle every
    residual is evaluated on in a cost sweep / the cached triangle a normal-equation sweep finds (-1: none; either may be None
    to leave that sweep out); weight: the edge weight; loss: index into LOSSES.  Returns a namespace with
      cost sweep    c_valid [m], c_r [m, 2], c_loss [m], cost, A_cost, n_cost
      normal eq.    valid [m], r [m, 2], w [m] (loss weight x edge weight), J [m, 2, 2B], packed [n_packed(B)], A [n_packed(B)], n_valid
    `mutant` plants one named error."""
    dtype = np.dtype(dtype).type
    loss = LOSSES.index(loss) if isinstance(loss, str) else int(loss)
    sp, tp = np.asarray(sp).astype(dtype).reshape(-1, 2), np.asarray(tp).astype(dtype).reshape(-1, 2)
    m = len(sp)
    V, T = geom.verts.astype(dtype), np.asarray(geom.tris).astype(np.int64)
    M, Mi = geom.model.astype(dtype), geom.model_inv.astype(dtype)
    Rs, ts, fxs, fys, cxs, cys, ars, s = _cam(dtype, cs)
    Rt, tt, fxt, fyt, cxt, cyt, art, st = _cam(dtype, ct)
    scale, wgt_e = dtype(scale), dtype(1.0 if mutant == "no_edge_weight" else weight)
    zero, one = np.zeros(m, dtype), np.ones(m, dtype)
    tgt_opencv = (st > 0) != (mutant == "tgt_behind_sign")
    out = SimpleNamespace()
    with np.errstate(all="ignore"):
        if prim_cost is not None:        # ---- Evaluate (refiner.cc:274-361) + TotalCost (lev_marq.h:773-824)
            found = np.asarray(prim_cost) >= 0
            idx = np.maximum(np.asarray(prim_cost), 0)
            o, d = source_rays(dtype, geom, cs, sp, mutant)
            _, t, _ = ray_triangle(dtype, o, d, V[T[idx, 0]], V[T[idx, 1]], V[T[idx, 2]])
            pw = _point(M, [o[k] + d[k] * t for k in range(3)])
            pc = [Rt[k, 0] * pw[0] + Rt[k, 1] * pw[1] + Rt[k, 2] * pw[2] + tt[k] for k in range(3)]
            behind = (pc[2] < 0) if tgt_opencv else (pc[2] > 0)
            rx, ry = fxt * pc[0] / pc[2] + cxt - tp[:, 0], fyt * pc[1] / pc[2] + cyt - tp[:, 1]
            valid = found & ~behind
            _, lv = _loss(dtype, loss, scale, rx * rx + ry * ry)
            lv = np.where(valid, lv, dtype(0))
            n = int(valid.sum())
            norm = dtype(n) if n else dtype(1)
            out.c_valid, out.c_r, out.c_loss, out.n_cost = valid, np.stack([rx, ry], 1), lv, n
            out.cost = wgt_e * (lv.sum(dtype=dtype) / norm)
            out.A_cost = float(wgt_e) * float(np.abs(lv).astype(np.float64).sum()) / max(n, 1)
        if prim_neq is not None:         # ---- EvaluateWithJacobian (refiner.cc:363-506) + BuildNormalEquations (lev_marq.h:653-771)
            N = 2 * B
            usable = np.asarray(prim_neq) >= 0
            idx = np.maximum(np.asarray(prim_neq), 0)
            origin = _center(Rs, ts)
            dc = [s * (sp[:, 0] - cxs) / fxs, s * (sp[:, 1] - cys) / fys, np.full(m, s, dtype)]
            dw = [Rs[0, k] * dc[0] + Rs[1, k] * dc[1] + Rs[2, k] * dc[2] for k in range(3)]      # DerotateWithJac
            p1, p2, p3 = V[T[idx, 0]], V[T[idx, 1]], V[T[idx, 2]]
            n_obj = _cross([p2[:, k] - p1[:, k] for k in range(3)], [p3[:, k] - p1[:, k] for k in range(3)])
            if mutant == "normal_not_transposed":
                nrm = [Mi[k, 0] * n_obj[0] + Mi[k, 1] * n_obj[1] + Mi[k, 2] * n_obj[2] for k in range(3)]
            else:                                                                                # normal = (model_inv^T)_3x3 n_obj
                nrm = [Mi[0, k] * n_obj[0] + Mi[1, k] * n_obj[1] + Mi[2, k] * n_obj[2] for k in range(3)]
            p0 = [M[k, 0] * p1[:, 0] + M[k, 1] * p1[:, 1] + M[k, 2] * p1[:, 2] + M[k, 3] for k in range(3)]
            # IntersectWithJac(ray, plane) (cpp/ray_casting.h:76-112)
            ddn = _dot(dw, nrm)
            gate = dtype(1e-10)
            ok = ~((ddn > -gate) & (ddn < gate))
            tpar = _dot([p0[k] - origin[k] for k in range(3)], nrm) / ddn
            inv_ddn = one / ddn
            X = [origin[k] + dw[k] * tpar for k in range(3)]
            A = [[(one if i == j else zero) - dw[i] * nrm[j] * inv_ddn for j in range(3)] for i in range(3)]   # dX/dO; dX/dDir = A t
            Xc = [Rt[k, 0] * X[0] + Rt[k, 1] * X[1] + Rt[k, 2] * X[2] + tt[k] for k in range(3)]
            behind = (Xc[2] < 0) if tgt_opencv else (Xc[2] > 0)
            rx, ry = fxt * Xc[0] / Xc[2] + cxt - tp[:, 0], fyt * Xc[1] / Xc[2] + cyt - tp[:, 1]
            d00, d02 = fxt / Xc[2], -fxt * Xc[0] / (Xc[2] * Xc[2])
            d11, d12 = fyt / Xc[2], -fyt * Xc[1] / (Xc[2] * Xc[2])
            G0 = [d00 * Rt[0, j] + d02 * Rt[2, j] for j in range(3)]                             # dp/dX = dp/dXCam R_t
            G1 = [d11 * Rt[1, j] + d12 * Rt[2, j] for j in range(3)]
            H0 = [G0[0] * A[0][j] + G0[1] * A[1][j] + G0[2] * A[2][j] for j in range(3)]         # dp/dX A
            H1 = [G1[0] * A[0][j] + G1[1] * A[1][j] + G1[2] * A[2][j] for j in range(3)]
            J0, J1 = [zero] * N, [zero] * N
            if not src_fixed:
                # H (Skew(origin) + t Skew(dirWorld)) = H Skew(origin + t dir);  H (-R_s^T)
                S = [[zero, -X[2], X[1]], [X[2], zero, -X[0]], [-X[1], X[0], zero]]
                for j in range(3):
                    J0[j] = H0[0] * S[0][j] + H0[1] * S[1][j] + H0[2] * S[2][j]
                    J1[j] = H1[0] * S[0][j] + H1[1] * S[1][j] + H1[2] * S[2][j]
                    J0[3 + j] = -(H0[0] * Rs[j, 0] + H0[1] * Rs[j, 1] + H0[2] * Rs[j, 2])
                    J1[3 + j] = -(H1[0] * Rs[j, 0] + H1[1] * Rs[j, 1] + H1[2] * Rs[j, 2])
                if B == 9:               # (H t) R_s^T dDirCam/d(fy, cx, cy), fx = fy * aspect  (UnprojectWithJac, types.h:100-125)
                    Q0 = [tpar * (H0[0] * Rs[j, 0] + H0[1] * Rs[j, 1] + H0[2] * Rs[j, 2]) for j in range(3)]
                    Q1 = [tpar * (H1[0] * Rs[j, 0] + H1[1] * Rs[j, 1] + H1[2] * Rs[j, 2]) for j in range(3)]
                    u00 = s * (cxs - sp[:, 0]) / (fys * fys if mutant == "no_aspect_src" else fys * fys * ars)
                    u01 = -s / fxs
                    u10, u12 = s * (cys - sp[:, 1]) / (fys * fys), -s / fys
                    if opt_f:
                        sg = dtype(-1.0 if mutant == "focal_sign_src" else 1.0)
                        J0[6], J1[6] = sg * (Q0[0] * u00 + Q0[1] * u10), sg * (Q1[0] * u00 + Q1[1] * u10)
                    if opt_pp:
                        a, b = (8, 7) if mutant == "pp_swapped" else (7, 8)
                        J0[a], J0[b], J1[a], J1[b] = Q0[0] * u01, Q0[1] * u12, Q1[0] * u01, Q1[1] * u12
            if not tgt_fixed:
                S = [[zero, X[2], -X[1]], [-X[2], zero, X[0]], [X[1], -X[0], zero]]              # Skew(-X)
                for j in range(3):
                    J0[B + j] = G0[0] * S[0][j] + G0[1] * S[1][j] + G0[2] * S[2][j]
                    J1[B + j] = G1[0] * S[0][j] + G1[1] * S[1][j] + G1[2] * S[2][j]
                J0[B + 3], J0[B + 5], J1[B + 4], J1[B + 5] = d00, d02, d11, d12
                if B == 9:
                    if opt_f:
                        J0[B + 6] = Xc[0] / Xc[2] if mutant == "no_aspect_tgt" else art * Xc[0] / Xc[2]
                        J1[B + 6] = Xc[1] / Xc[2]
                    if opt_pp:
                        a, b = (8, 7) if mutant == "pp_swapped" else (7, 8)
                        J0[B + a], J1[B + b] = one, one
            lw, _ = _loss(dtype, loss, scale, rx * rx + ry * ry, mutant)
            valid = ok & ~behind & usable
            w = np.where(valid, wgt_e * lw, dtype(0))
            J0 = [np.where(valid, c, dtype(0)) for c in J0]
            J1 = [np.where(valid, c, dtype(0)) for c in J1]
            wrx, wry = np.where(valid, w * rx, dtype(0)), np.where(valid, w * ry, dtype(0))
            n = int(valid.sum())
            norm = dtype(n) if n else dtype(1)
            TR = tril(B)
            packed = [(w * (J0[p] * J0[q] + J1[p] * J1[q])).sum(dtype=dtype) / norm for p, q in TR]
            packed += [(J0[p] * wrx + J1[p] * wry).sum(dtype=dtype) / norm for p in range(N)]
            a64 = lambda v: np.abs(v).astype(np.float64)   # noqa: E731
            Aabs = [float((a64(w) * (a64(J0[p]) * a64(J0[q]) + a64(J1[p]) * a64(J1[q]))).sum()) / max(n, 1) for p, q in TR]
            Aabs += [float((a64(J0[p]) * a64(wrx) + a64(J1[p]) * a64(wry)).sum()) / max(n, 1) for p in range(N)]
            out.valid, out.r, out.w, out.n_valid = valid, np.stack([rx, ry], 1), w, n
            out.J = np.stack([np.stack(J0, 1), np.stack(J1, 1)], 1)
            out.packed, out.A = np.array(packed, dtype), np.array(Aabs)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# triangle choice
# ---------------------------------------------------------------------------------------------------------------------
def select_triangles(dtype, geom, sweeps, kp_offset, kp_xy, mask=None):
    """Steps the per-keypoint cache through the sweeps ((kind, cameras), kind "cost" or "neq") in `dtype`.  Returns
      used    per sweep [n_kp]: cost -- the triangle the residual is evaluated on (-1: none); neq -- the cached triangle
      margin  [n_kp] smallest float64 barycentric margin of any decision taken for the keypoint (closest hit over the mesh, and
              hit-or-miss of the cached triangle)
      gap     [n_kp] smallest gap in t between a closest hit and its runner-up
      closest per sweep [n_kp]: the closest hit itself (cost sweeps; what a cold cache would give)"""
    n_frames = len(kp_offset) - 1
    V, T = geom.verts, np.asarray(geom.tris).astype(np.int64)
    cache = np.full(len(kp_xy), -1)
    margin, gap = np.full(len(kp_xy), np.inf), np.full(len(kp_xy), np.inf)
    used, closest = [], []
    for kind, cams in sweeps:
        if kind == "neq":
            used.append(cache.copy())
            closest.append(None)
            continue
        near = np.full(len(kp_xy), -1)
        for f in range(n_frames):
            sl = slice(kp_offset[f], kp_offset[f + 1])
            if sl.start == sl.stop:
                continue
            o, d = source_rays(dtype, geom, cams[f], kp_xy[sl])
            r = tr.mt_closest(dtype, V, T, np.array(o), np.stack(d, 1))
            best = r.prim.copy()
            if mask is not None:
                best[(best >= 0) & mask[np.maximum(best, 0)]] = -1
            prev = cache[sl]
            has = prev >= 0
            idx = np.maximum(prev, 0)
            Vd = V.astype(dtype)
            hit_c, _, m_c = ray_triangle(dtype, o, d, Vd[T[idx, 0]], Vd[T[idx, 1]], Vd[T[idx, 2]])
            keep = has & hit_c
            cache[sl] = np.where(keep, prev, best)
            near[sl] = r.prim
            margin[sl] = np.minimum(margin[sl], np.minimum(r.m_bary, np.where(has, m_c, np.inf)))
            gap[sl] = np.minimum(gap[sl], r.m_t)
        used.append(cache.copy())
        closest.append(near)
    return SimpleNamespace(used=used, margin=margin, gap=gap, closest=closest)


# ---------------------------------------------------------------------------------------------------------------------
# named cases
# ---------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385, 511, 512, 513, 769, 1025)
SIZES_CASE_EDGES = EDGE_SIZES + (64,)      # the edge of weight 0 is one more edge: every size above is compared at a weight that counts
CX, CY, F = 470.0, 281.5, 1100.0


def two_triangle_mesh():
    """a large back triangle (index 0) and a small front triangle (index 1) one unit nearer to a camera on the +z side"""
    verts = np.array([[-8, -6, 0], [8, -6, 0], [0, 10, 0], [0.2, -0.3, 1], [1.0, -0.3, 1], [0.6, 0.5, 1]], np.float32)
    return verts, np.array([[0, 1, 2], [3, 4, 5]], np.uint32)


def cameras(n_frames, opencv, aspect, shift=(0.0, 0.0, 0.0), turned=()):
    """a camera 8 units in front of the mesh, drifting and turning a little from frame to frame; focal length and principal
    point differ between frames, the principal point is off-centre; `turned` frames look the other way"""
    out = []
    for f in range(n_frames):
        k = f - (n_frames - 1) / 2
        R = tr._rot([0.1, 1.0, 0.3], 0.02 * k) @ tr._rot([0.2, 1.0, 0.1], 0.05) @ tr._rot([1, 0, 0], 0.03)
        t = np.array([0.05 + 0.06 * k, -0.04 - 0.03 * k, -8.0 + 0.05 * f]) + np.asarray(shift)
        if f in turned:
            flip = np.diag([-1.0, 1.0, -1.0])
            R, t = flip @ R, flip @ t
        if opencv:                                   # the same camera seen as OpenCV: y and z of the view flip
            flip = np.diag([1.0, -1.0, -1.0])
            R, t = flip @ R, flip @ t
        fy = (F if opencv else -F) * (1 + 0.004 * f)
        out.append(make_camera(R, t, fy, aspect, CX + 1.5 * f, CY - f, opencv))
    return out


def _project(cam, Xw):
    Z = Xw @ cam.R.T + cam.t
    return np.stack([cam.fx * Z[:, 0] / Z[:, 2] + cam.cx, cam.fy * Z[:, 1] / Z[:, 2] + cam.cy], 1)


def _neighbour_edges(n_frames, skips=(-2, -1, 1, 2)):
    return [(i, i + s) for i in range(n_frames) for s in skips if 0 <= i + s < n_frames]


def case_specs():
    """name -> keyword arguments of make_case: the one table the CPU and the GPU file are driven by"""
    specs = {}
    table = (("rot_scale", False, 0.8, "huber", True, True), ("rot_scale", True, 1.07, "cauchy", False, False),
             ("shear", False, 1.07, "trivial", False, False), ("shear", True, 0.8, "huber", True, False),
             ("mirror", False, 0.8, "cauchy", False, True), ("mirror", True, 1.07, "huber", False, False),
             ("diagonal", False, 0.8, "cauchy", False, False), ("diagonal", True, 1.07, "trivial", True, True))
    for kind, opencv, aspect, loss, opt_f, opt_pp in table:
        specs[f"{kind}-{'opencv' if opencv else 'opengl'}"] = dict(matrix=kind, opencv=opencv, aspect=aspect, loss=loss, opt_f=opt_f, opt_pp=opt_pp)
    specs["sizes-b6"] = dict(matrix="rot_scale", opencv=True, aspect=1.07, loss="huber", opt_f=False, opt_pp=False, layout="sizes")
    specs["sizes-b9"] = dict(matrix="shear", opencv=False, aspect=0.8, loss="cauchy", opt_f=True, opt_pp=True, layout="sizes")
    specs["target-turned-away"] = dict(matrix="shear", opencv=True, aspect=0.8, loss="cauchy", opt_f=True, opt_pp=False, turned=(3,))
    specs["cache-across-sweeps"] = dict(matrix="rot_scale", opencv=False, aspect=1.07, loss="huber", opt_f=False, opt_pp=True,
                                        n_frames=4, order=("cost", "cost_b", "neq_b"), shift=(0.05, -0.03, 0.0))
    specs["normal-equations-first"] = dict(matrix="mirror", opencv=True, aspect=0.8, loss="trivial", opt_f=True, opt_pp=True,
                                           n_frames=4, order=("neq", "cost", "neq"))
    specs["cached-triangle-kept"] = dict(matrix="diagonal", opencv=False, aspect=1.07, loss="huber", opt_f=False, opt_pp=False,
                                         n_frames=4, order=("cost", "cost_b", "neq_b"), shift=(1.5, 0.0, 0.0), mesh="two", off_share=0.0)
    # the one scene that also goes through polychase_core (all keypoints on the mesh: the bounding-box filter keeps them all)
    specs["core-rot_scale"] = dict(matrix="rot_scale", opencv=False, aspect=0.8, loss="huber", opt_f=True, opt_pp=True, off_share=0.0, n_kp=200)
    return specs


def make_case(name, matrix, opencv, aspect, loss, opt_f, opt_pp, layout="neighbours", n_frames=5, n_kp=260, order=("cost", "neq"),
              shift=None, turned=(), mesh="grid", off_share=0.1, scale=1.0):
    """One named problem.  Keypoints are constructed: a triangle and barycentric coordinates at least 0.05 from every edge, through
    the model matrix, projected by the source camera, rounded to float32; off-mesh keypoints (off_share) are projections of
    points beside the mesh.  A candidate is kept only if every decision taken for it in every cost sweep has the float64 margin
    MARGIN (closest hit or miss over all triangles, hit or miss of the cached triangle) and a positive gap in t -- and, where the
    camera looks at the mesh, the closest hit of the first sweep is the triangle it was drawn on.  Targets: the point seen by the
    target camera + N(0, 0.5 px), one in twenty an outlier of 5-30 px."""
    names = sorted(case_specs())
    rng = np.random.default_rng(1000 + names.index(name))
    model = tr.raycast_scene_specs()[f"{matrix}-opengl"][0]
    geom = SimpleNamespace(model=model.astype(np.float64), model_inv=np.linalg.inv(model.astype(np.float64)).astype(np.float32).astype(np.float64))
    geom.verts, geom.tris = two_triangle_mesh() if mesh == "two" else tr.grid_mesh()
    B = 9 if (opt_f or opt_pp) else 6
    cams_a = cameras(n_frames, opencv, aspect, turned=turned)
    cams_b = cameras(n_frames, opencv, aspect, shift=shift, turned=turned) if shift is not None else None
    sweeps = [("neq" if s.startswith("neq") else "cost", cams_b if s.endswith("_b") else cams_a) for s in order]
    cost_sweeps = [sw for sw in sweeps if sw[0] == "cost"]
    V64, T = geom.verts.astype(np.float64), geom.tris.astype(np.int64)
    if layout == "sizes":
        n_kp = 1100
    # candidates, more than needed; the margins choose
    n_cand = int(n_kp * 1.5) + 8
    kps, worlds, on_mesh = [], [], []
    for f in range(n_frames):
        n_off = int(round(off_share * n_cand))
        if mesh == "two":     # points of the FRONT triangle seen by camera B: at A the same pixel sees the back triangle beside it
            tri = np.ones(n_cand, np.int64)
            draw_cam = cams_b[f]
        else:
            tri = rng.integers(0, len(T), n_cand)
            draw_cam = cams_a[f]
        bary = 0.05 + 0.85 * rng.dirichlet([1, 1, 1], n_cand)
        P = (bary[:, :, None] * V64[T[tri]]).sum(1)
        if n_off:
            side = rng.uniform(2.3, 3.0, n_off) * rng.choice([-1, 1], n_off)
            other = rng.uniform(-3.0, 3.0, n_off)
            flip = rng.uniform(size=n_off) < 0.5
            P[:n_off] = np.stack([np.where(flip, side, other), np.where(flip, other, side), np.zeros(n_off)], 1)
        Pw = P @ geom.model[:3, :3].T + geom.model[:3, 3]
        xy = _project(draw_cam, Pw).astype(np.float32)
        off = np.arange(n_cand) < n_off
        # select_triangles indexes cameras by frame: hand it this frame's camera as frame 0
        sel = select_triangles(np.float64, geom, [(k, [c[f]]) for k, c in cost_sweeps], np.array([0, n_cand]), xy)
        safe = (sel.margin >= MARGIN) & (sel.gap > 0)
        first = sel.closest[0]
        if mesh == "two":
            safe &= (first == 0) & (sel.closest[1] == 1)
        elif f in turned:
            safe &= first == -1
        else:
            safe &= np.where(off, first == -1, first == tri)
        keep_off = np.nonzero(safe & off)[0][:int(round(off_share * n_kp))]
        keep = np.concatenate([keep_off, np.nonzero(safe & ~off)[0][:n_kp - len(keep_off)]])
        assert len(keep) == n_kp, (name, f, len(keep))
        keep = rng.permutation(keep)               # on- and off-mesh keypoints mixed
        kps.append(xy[keep])
        worlds.append(Pw[keep])
        on_mesh.append(~off[keep])
    kp_offset = np.arange(n_frames + 1, dtype=np.int32) * n_kp
    kp_xy = np.concatenate(kps).astype(np.float32)
    # edges
    if layout == "sizes":
        pairs = [(1, 2), (2, 1), (0, 1), (1, 0), (2, 3), (3, 2), (4, 3), (3, 4), (1, 3), (3, 1)]
        edges = [(pairs[k % len(pairs)] + (size,)) for k, size in enumerate(SIZES_CASE_EDGES)]
        weights = [(1.0, 0.5, 1.0 / 3.0)[k % 3] for k in range(len(edges))]
        weights[-1] = 0.0
    else:
        edges = [(i, j, int(0.8 * n_kp)) for i, j in _neighbour_edges(n_frames)]
        weights = [1.0 / (min(i, n_frames - 1 - i) + 1.0) for i, _, _ in edges]      # FrameWeight(image_id_from)
    cams_t = sweeps[-1][1]
    src, tgt, off, res_kp, res_xy = [], [], [0], [], []
    for i, j, size in edges:
        take = rng.permutation(n_kp)[:size].astype(np.uint32)       # a random permutation, not sorted
        x2 = _project(cams_t[j], worlds[i][take]) + rng.normal(0, 0.5, (size, 2))
        outl = rng.uniform(size=size) < 0.05
        ang, mag = rng.uniform(0, 2 * np.pi, size), rng.uniform(5, 30, size)
        x2[outl] += (mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))[outl]
        x2 = np.where(on_mesh[i][take, None], x2, kps[i][take] + 1.0 + rng.normal(0, 0.5, (size, 2)))
        src.append(i)
        tgt.append(j)
        res_kp.append(take)
        res_xy.append(x2.astype(np.float32))
        off.append(off[-1] + size)
    return SimpleNamespace(
        name=name, geom=geom, mesh=mesh, B=B, opt_f=bool(opt_f), opt_pp=bool(opt_pp), loss=LOSSES.index(loss), scale=float(np.float32(scale)),
        opencv=opencv, aspect=aspect, matrix=matrix, n_frames=n_frames, sweeps=sweeps, order=order, kp_offset=kp_offset, kp_xy=kp_xy,
        edge_src=np.array(src, np.int32), edge_tgt=np.array(tgt, np.int32), edge_offset=np.array(off, np.int32),
        res_src_kp=np.concatenate(res_kp).astype(np.uint32), res_tgt_xy=np.concatenate(res_xy).astype(np.float32).reshape(-1, 2),
        edge_weight=np.array(weights, np.float32), on_mesh=np.concatenate(on_mesh), turned=tuple(turned))


def evaluate(dtype, case, sel, mutant=None):
    """every sweep of the case in `dtype` on the triangles `sel` names -> per sweep a namespace: kind, valid [E], and for a cost
    sweep cost [E], A_cost [E], total; for a normal-equation sweep packed [E, n_packed], A [E, n_packed]"""
    E = len(case.edge_src)
    out = []
    for (kind, cams), used in zip(case.sweeps, sel.used):
        res = SimpleNamespace(kind=kind, valid=np.zeros(E, np.int64))
        if kind == "cost":
            res.cost, res.A_cost = np.zeros(E, dtype), np.zeros(E)
        else:
            res.packed, res.A = np.zeros((E, n_packed(case.B)), dtype), np.zeros((E, n_packed(case.B)))
        for e in range(E):
            i, j = int(case.edge_src[e]), int(case.edge_tgt[e])
            sl = slice(case.edge_offset[e], case.edge_offset[e + 1])
            kp = case.kp_offset[i] + case.res_src_kp[sl].astype(np.int64)
            prim = used[kp]
            t = edge_terms(dtype, case.geom, cams[i], cams[j], case.kp_xy[kp], case.res_tgt_xy[sl], prim if kind == "cost" else None,
                           prim if kind == "neq" else None, float(case.edge_weight[e]), case.loss, case.scale, case.B, case.opt_f, case.opt_pp,
                           i in (0, case.n_frames - 1), j in (0, case.n_frames - 1), mutant)
            if kind == "cost":
                res.valid[e], res.cost[e], res.A_cost[e] = t.n_cost, t.cost, t.A_cost
            else:
                res.valid[e], res.packed[e], res.A[e] = t.n_valid, t.packed, t.A
        if kind == "cost":
            res.total = float(res.cost.astype(np.float64).sum())
        out.append(res)
    return out


def rho_of(r32, r64, B):
    """(rho_tri, rho_grad, rho_cost) of one case's float32 run against its float64 run; where A_k is 0 both have to be exactly 0"""
    nt = (2 * B) * (2 * B + 1) // 2
    rho = [0.0, 0.0, 0.0]
    for a, b in zip(r32, r64):
        if b.kind == "cost":
            parts = ((2, a.cost, b.cost, b.A_cost),)
        else:
            parts = ((0, a.packed[:, :nt], b.packed[:, :nt], b.A[:, :nt]), (1, a.packed[:, nt:], b.packed[:, nt:], b.A[:, nt:]))
        for k, got, want, A in parts:
            got = np.asarray(got, np.float64)
            live = A > 0
            assert np.all(got[~live] == 0) and np.all(want[~live] == 0)
            if live.any():
                rho[k] = max(rho[k], float((np.abs(got[live] - want[live]) / (EPS24 * A[live])).max()))
    return tuple(rho)


def scatter(case, packed, B=None):
    """the per-edge blocks added into the dense system the way the host assembles them: edges of weight 0 are left out,
    JtJ comes back full and symmetric.  Works on values and on bounds alike."""
    B = case.B if B is None else B
    n, nt = case.n_frames * B, (2 * B) * (2 * B + 1) // 2
    JtJ, Jtr = np.zeros((n, n)), np.zeros(n)
    for e in range(len(case.edge_src)):
        if case.edge_weight[e] == 0:
            continue
        at = np.concatenate([int(case.edge_src[e]) * B + np.arange(B), int(case.edge_tgt[e]) * B + np.arange(B)])
        for k, (a, b) in enumerate(tril(B)):
            JtJ[at[a], at[b]] += packed[e, k]
            if at[a] != at[b]:
                JtJ[at[b], at[a]] += packed[e, k]
        Jtr[at] += packed[e, nt:]
    return JtJ, Jtr


_cache = {}


def reference(name):
    """(case, float64 triangle choice, float64 sweeps, rho of the float32 restatement) of a named case, once per process"""
    if name not in _cache:
        case = make_case(name, **case_specs()[name])
        sel = select_triangles(np.float64, case.geom, case.sweeps, case.kp_offset, case.kp_xy)
        r64 = evaluate(np.float64, case, sel)
        r32 = evaluate(np.float32, case, sel)
        assert all(np.array_equal(a.valid, b.valid) for a, b in zip(r32, r64)), name
        _cache[name] = (case, sel, r64, rho_of(r32, r64, case.B))
    return _cache[name]


def rho_worst():
    """the three worst rho over the whole case list"""
    rho = np.array([reference(name)[3] for name in case_specs()])
    return tuple(float(v) for v in rho.max(0))
