"""CPU: the float64 / float32 restatement of the refiner's two sweeps (tests/refiner_ref.py) is checked against the oracle and
against finite differences, the float32 noise the GPU bound is made of is measured and recorded
(profiles/refiner_edge_noise.txt), the bound is shown to notice planted errors today's tolerances of tests/test_refiner_gpu.py
let through, and every named case is shown to decide its triangles with a margin float32 cannot cross
(tests/test_refine_edges_gpu.py applies the bound to the kernels)."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_oracle as po  # noqa: E402
import refine_oracle as ro  # noqa: E402
import refiner_ref as rr  # noqa: E402
import tracker_ref as tr  # noqa: E402

SPECS = rr.case_specs()


def _record(name, lines):
    path = os.path.join(ROOT, "profiles", name)
    text = "\n".join(lines) + "\n"
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)


class _MatrixCamera(po.Camera):
    """the oracle's camera with the rotation given as the matrix the kernel gets (no trip through a quaternion)"""
    Rm = None

    def R(self):
        return self.Rm


def _oracle_camera(c):
    cam = _MatrixCamera(fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy, aspect_ratio=c.aspect, width=960.0, height=540.0, opencv=c.sign > 0, t=c.t)
    cam.Rm = c.R
    return cam


def _oracle_segment(case):
    kps = [case.kp_xy[case.kp_offset[f]:case.kp_offset[f + 1]].astype(np.float64) for f in range(case.n_frames)]
    edges = [(int(case.edge_src[e]), int(case.edge_tgt[e]), case.res_src_kp[case.edge_offset[e]:case.edge_offset[e + 1]].astype(np.int64),
              case.res_tgt_xy[case.edge_offset[e]:case.edge_offset[e + 1]].astype(np.float64), float(case.edge_weight[e]))
             for e in range(len(case.edge_src))]
    return ro.Segment(0, case.n_frames, kps, edges, [np.full(len(k), ro.INVALID) for k in kps])


@pytest.mark.parametrize("name", ["rot_scale-opengl", "shear-opencv", "mirror-opengl", "diagonal-opencv", "target-turned-away"])
def test_restatement_equals_the_oracle(name):
    """the same residuals, Jacobians, normal equations and cost to 1e-12 relative, on a small edition of the named case (the
    oracle walks its residuals one by one) and with the exact float64 inverse of the model matrix, which is what the oracle uses"""
    case = rr.make_case(name, **{**SPECS[name], "n_kp": 60})
    case.geom = copy.copy(case.geom)
    case.geom.model_inv = np.linalg.inv(case.geom.model)
    sel = rr.select_triangles(np.float64, case.geom, case.sweeps, case.kp_offset, case.kp_xy)
    r64 = rr.evaluate(np.float64, case, sel)
    g, cams = case.geom, [_oracle_camera(c) for c in case.sweeps[0][1]]
    seg = _oracle_segment(case)
    mask = np.zeros((len(g.tris) + 31) // 32, np.uint32)
    kind = rr.LOSSES[case.loss]
    cost = ro.total_cost(seg, cams, g.verts, g.tris, mask, g.model, kind, case.scale)
    assert r64[0].total == pytest.approx(cost, rel=1e-12)
    for f in range(case.n_frames):                               # the oracle's cache is the triangle choice (where an edge asked)
        asked = np.unique(np.concatenate([e[2] for e in seg.edges if e[0] == f]))
        assert np.array_equal(seg.cache[f][asked], sel.used[0][case.kp_offset[f] + asked])
    JtJ, Jtr = ro.normal_equations(seg, cams, g.verts, g.tris, g.model, kind, case.scale, case.opt_f, case.opt_pp)
    got_JtJ, got_Jtr = rr.scatter(case, r64[1].packed)
    assert np.allclose(got_JtJ, JtJ, rtol=1e-12, atol=1e-12 * np.abs(JtJ).max())
    assert np.allclose(got_Jtr, Jtr, rtol=1e-12, atol=1e-12 * np.abs(Jtr).max())
    # per residual, two edges: free -> free and one with a fixed end
    for e in (0, len(seg.edges) // 2):
        i, j, kp_idx, tgt, w = seg.edges[e]
        prim = sel.used[0][case.kp_offset[i] + kp_idx]
        t = rr.edge_terms(np.float64, g, case.sweeps[0][1][i], case.sweeps[0][1][j], seg.kps[i][kp_idx], tgt, prim, prim, w, case.loss, case.scale,
                          case.B, case.opt_f, case.opt_pp, i in (0, case.n_frames - 1), j in (0, case.n_frames - 1))
        r, valid = ro.edge_residuals(seg, cams, e, g.verts, g.tris, mask, g.model)
        assert np.array_equal(valid, t.c_valid) and np.allclose(t.c_r[valid], r[valid], rtol=0, atol=1e-12 * 1000)
        J, r, valid = ro.edge_jacobians(seg, cams, e, g.verts, g.tris, g.model, case.opt_f, case.opt_pp)
        assert np.array_equal(valid, t.valid) and np.allclose(t.r[valid], r[valid], rtol=0, atol=1e-12 * 1000)
        assert np.allclose(t.J[valid], J[valid], rtol=1e-12, atol=1e-12 * np.abs(J).max())
        assert valid.any() or name == "target-turned-away"


@pytest.mark.parametrize("name", ["shear-opengl", "shear-opencv"])
def test_jacobian_equals_central_differences(name):
    """all 18 columns with aspect != 1 and a sheared model matrix: rotation (applied on the right like QuatStepPost), translation,
    fy (fx = aspect * fy), cx, cy of the source and of the target camera"""
    case = rr.reference(name)[0]
    sel = rr.reference(name)[1]
    e = 4
    i, j = int(case.edge_src[e]), int(case.edge_tgt[e])
    assert i not in (0, case.n_frames - 1) and j not in (0, case.n_frames - 1) and case.aspect != 1.0
    sl = slice(case.edge_offset[e], case.edge_offset[e + 1])
    kp = case.kp_offset[i] + case.res_src_kp[sl].astype(np.int64)
    prim = sel.used[0][kp]
    cs, ct = case.sweeps[0][1][i], case.sweeps[0][1][j]

    def terms(cs_, ct_):
        return rr.edge_terms(np.float64, case.geom, cs_, ct_, case.kp_xy[kp], case.res_tgt_xy[sl], None, prim, 1.0, "trivial", 1.0, 9, True, True,
                             False, False)

    def moved(c, d):
        q = copy.copy(c)
        ang = np.linalg.norm(d[:3])
        q.R = c.R @ (tr._rot(d[:3], ang) if ang > 0 else np.eye(3))
        q.t = c.t + d[3:6]
        q.fy, q.fx, q.cx, q.cy = c.fy + d[6], c.fx + c.aspect * d[6], c.cx + d[7], c.cy + d[8]
        return q

    base = terms(cs, ct)
    ok = base.valid
    assert ok.sum() > 100
    h = 1e-5
    for k in range(18):
        d = np.zeros(9)
        d[k % 9] = h
        plus, minus = (terms(moved(cs, d), ct), terms(moved(cs, -d), ct)) if k < 9 else (terms(cs, moved(ct, d)), terms(cs, moved(ct, -d)))
        fd = (plus.r - minus.r) / (2 * h)
        col = base.J[:, :, k]
        assert np.allclose(col[ok], fd[ok], rtol=1e-6, atol=1e-6 * np.abs(col[ok]).max()), k
    assert np.abs(base.J[ok][:, 0, 6]).max() > 1e-3 and np.abs(base.J[ok][:, 0, 15]).max() > 0.05     # the focal columns are there


def test_every_case_decides_its_triangles_with_a_margin_and_float32_agrees():
    """for every kept keypoint of every case: every decision of every cost sweep has the float64 margin, and the float32
    restatement of the ray cast steps the cache through the same triangles -- so edge_valid can be required to be equal"""
    worst, rays = np.inf, 0
    for name in SPECS:
        case, sel, r64, _ = rr.reference(name)
        s32 = rr.select_triangles(np.float32, case.geom, case.sweeps, case.kp_offset, case.kp_xy)
        for a, b in zip(s32.used, sel.used):
            assert np.array_equal(a, b), name
        assert sel.margin.min() >= rr.MARGIN and sel.gap.min() > 0, name
        worst, rays = min(worst, float(sel.margin.min())), rays + len(case.kp_xy) * sum(k == "cost" for k, _ in case.sweeps)
        assert len(case.res_src_kp) <= 8500 and case.n_frames in (4, 5), name
        # the residuals of an edge are not sorted by keypoint
        big = int(np.argmax(np.diff(case.edge_offset)))
        kp = case.res_src_kp[case.edge_offset[big]:case.edge_offset[big + 1]]
        assert np.any(np.diff(kp.astype(np.int64)) < 0), name
    print(f"{rays} rays, smallest float64 margin {worst:.4f}")


def test_the_case_table_holds_what_it_promises():
    kinds = {}
    for name in SPECS:
        case = rr.reference(name)[0]
        kinds.setdefault(case.matrix, set()).add((case.B, case.opencv, case.aspect))
    for kind in ("rot_scale", "shear", "mirror", "diagonal"):
        assert {b for b, _, _ in kinds[kind]} == {6, 9} and {cv for _, cv, _ in kinds[kind]} == {False, True}, kind
    assert {a for v in kinds.values() for _, _, a in v} == {0.8, 1.07}
    table = [rr.reference(n)[0] for n in SPECS if "-open" in n]
    assert {c.loss for c in table} == {0, 1, 2} and {(c.opt_f, c.opt_pp) for c in table} == {(False, False), (True, False), (False, True), (True, True)}
    # edge sizes: every size, for both block lengths; all four kinds of ends; the weights; about a tenth of the keypoints off the mesh
    for name, B in (("sizes-b6", 6), ("sizes-b9", 9)):
        case, sel, r64, _ = rr.reference(name)
        assert case.B == B and tuple(np.diff(case.edge_offset)) == rr.SIZES_CASE_EDGES and set(rr.EDGE_SIZES) == set(rr.SIZES_CASE_EDGES)
        last = case.n_frames - 1
        ends = {(int(s) in (0, last), int(t) in (0, last)) for s, t in zip(case.edge_src, case.edge_tgt)}
        assert ends == {(False, False), (True, False), (False, True)}
        free = [(int(s), int(t)) for s, t in zip(case.edge_src, case.edge_tgt) if s not in (0, last) and t not in (0, last)]
        assert any(s < t for s, t in free) and any(s > t for s, t in free)
        assert set(np.float32([1.0, 0.5, 1.0 / 3.0, 0.0])) == set(case.edge_weight) and (case.edge_weight == 0).sum() == 1
        assert (case.edge_weight[:len(rr.EDGE_SIZES)] > 0).all()              # every size is compared at a weight that counts
        assert 0.05 < (~case.on_mesh).mean() < 0.15
        big = r64[1].valid[rr.EDGE_SIZES.index(1025)]
        assert 0.8 * 1025 < big < 1025                       # invalid residuals inside an edge
    # the target camera that looks away: every edge into it and out of it is empty, the others are not
    case, sel, r64, _ = rr.reference("target-turned-away")
    into = (case.edge_tgt == 3) | (case.edge_src == 3)
    assert into.sum() >= 4 and not r64[0].valid[into].any() and not r64[1].valid[into].any() and r64[1].valid[~into].min() > 100
    assert not r64[1].packed[into].any() and not r64[0].cost[into].any()
    # an edge into it whose rays DO hit: it is the target's side that empties it
    e = int(np.nonzero((case.edge_tgt == 3) & (case.edge_src != 3))[0][0])
    kp = case.kp_offset[case.edge_src[e]] + case.res_src_kp[case.edge_offset[e]:case.edge_offset[e + 1]].astype(np.int64)
    assert (sel.used[0][kp] >= 0).mean() > 0.8
    # the cache across sweeps: a good share of the rays leave their triangle, some keep it
    case, sel, r64, _ = rr.reference("cache-across-sweeps")
    hit = sel.used[0] >= 0
    moved = (sel.used[0] != sel.used[1]) & hit
    print("cache-across-sweeps: rays that leave their triangle", moved.sum(), "of", hit.sum())
    assert 0.2 * hit.sum() < moved.sum() < 0.95 * hit.sum()
    assert np.array_equal(sel.used[2], sel.used[1]) and [k for k, _ in case.sweeps] == ["cost", "cost", "neq"]
    # normal equations before any cost sweep: nothing is cached, everything is zero; afterwards it is not
    case, sel, r64, _ = rr.reference("normal-equations-first")
    assert [k for k, _ in case.sweeps] == ["neq", "cost", "neq"] and (sel.used[0] == -1).all()
    assert not r64[0].valid.any() and not r64[0].packed.any() and not r64[0].A.any() and r64[2].valid.min() > 100
    # the cached back triangle is kept although the front triangle now covers it
    case, sel, r64, _ = rr.reference("cached-triangle-kept")
    assert (sel.used[0] == 0).all() and (sel.closest[1] == 1).all() and (sel.used[1] == 0).all() and (sel.used[2] == 0).all()
    assert r64[2].valid.min() > 100


def test_float32_noise_is_measured_and_recorded_and_the_bound_rejects_every_mutant():
    """rho per class over every named case; GPU bound per entry = BOUND_FACTOR * rho * 2^-24 * A_k.  Every mutant breaks it on its
    named case, the unmutated float32 restatement does not; for four of them today's assertions of tests/test_refiner_gpu.py are
    applied to the mutated result and the verdict is recorded (it documents the gap, it is not asserted)."""
    rows = [(name, rr.reference(name)[3]) for name in SPECS]
    worst = rr.rho_worst()
    at = [max(rows, key=lambda r: r[1][k])[0] for k in range(3)]
    lines = ["float32 restatement against float64, rho = max_k |v32_k - v64_k| / (2^-24 * A_k), A_k = sum_i |term_i| / n_valid, tests/refiner_ref.py",
             f"cases {len(rows)}",
             f"rho_triangle {worst[0]:.3f}  at {at[0]}", f"rho_gradient {worst[1]:.3f}  at {at[1]}", f"rho_cost     {worst[2]:.3f}  at {at[2]}",
             f"GPU bound per entry = {tr.BOUND_FACTOR:g} * rho * 2^-24 * A_k = "
             f"{tr.BOUND_FACTOR * worst[0] * tr.EPS24:.2e} / {tr.BOUND_FACTOR * worst[1] * tr.EPS24:.2e} / {tr.BOUND_FACTOR * worst[2] * tr.EPS24:.2e} of A_k",
             "case                      rho_triangle  rho_gradient  rho_cost"]
    lines += [f"{name:24s}  {r[0]:12.3f}  {r[1]:12.3f}  {r[2]:8.3f}" for name, r in rows]
    assert all(np.isfinite(worst)) and all(w > 0 for w in worst)
    # a bound of more than 1e-2 of the absolute sum would notice nothing
    assert tr.BOUND_FACTOR * max(worst) * tr.EPS24 < 1e-2
    lines.append("mutant                      case                  new bound   worst |v - f64| / bound   block Frobenius 2e-3 / Jtr norm 2e-3 of today")
    for mutant in rr.MUTANTS:
        name = MUTANT_CASES[mutant]
        clean, _ = _against_the_bound(name, None, worst)
        broken, ratio = _against_the_bound(name, mutant, worst)
        old = _todays_assertions(name, mutant) if mutant in OLD_TOLERANCE_MUTANTS else "-"
        lines.append(f"{mutant:26s}  {name:20s}  {'rejected' if broken else 'PASSES'}    {ratio:12.1f}              {old}")
        assert not clean, (name, "the float32 restatement itself breaks the bound")
        assert broken, mutant
    lines.append("(normal_not_transposed is noticed by today's tolerances on this model matrix -- the scenes of tests/test_refiner_gpu.py "
                 "use diagonal ones, where the mutant changes nothing)")
    print("\n".join(lines))
    _record("refiner_edge_noise.txt", lines)


MUTANT_CASES = {"no_aspect_src": "rot_scale-opengl", "no_aspect_tgt": "rot_scale-opengl", "focal_sign_src": "diagonal-opencv",
                "normal_not_transposed": "rot_scale-opencv", "dir_not_through_model_inv": "shear-opengl", "pp_swapped": "mirror-opengl",
                "tgt_behind_sign": "mirror-opencv", "no_edge_weight": "rot_scale-opengl", "huber_r2": "mirror-opencv"}
OLD_TOLERANCE_MUTANTS = ("no_aspect_src", "no_aspect_tgt", "focal_sign_src", "normal_not_transposed")


def _against_the_bound(name, mutant, rho):
    """(breaks the bound, worst ratio to it) of the float32 restatement with `mutant` planted"""
    case, sel, r64, _ = rr.reference(name)
    got = rr.evaluate(np.float32, case, sel, mutant)
    nt = (2 * case.B) * (2 * case.B + 1) // 2
    broken, worst = False, 0.0
    for a, b in zip(got, r64):
        broken |= not np.array_equal(a.valid, b.valid)
        if b.kind == "cost":
            parts = ((a.cost, b.cost, b.A_cost, rho[2]),)
        else:
            parts = ((a.packed[:, :nt], b.packed[:, :nt], b.A[:, :nt], rho[0]), (a.packed[:, nt:], b.packed[:, nt:], b.A[:, nt:], rho[1]))
        for g, want, A, r in parts:
            err = np.abs(np.asarray(g, np.float64) - want)
            bound = tr.BOUND_FACTOR * r * tr.EPS24 * A
            broken |= bool((err > bound).any())
            live = A > 0
            if live.any():
                worst = max(worst, float((err[live] / bound[live]).max()))
    return broken, worst


def _todays_assertions(name, mutant):
    """tests/test_refiner_gpu.py::test_cost_and_normal_equations_match_oracle applied to the mutated float32 result"""
    case, sel, r64, _ = rr.reference(name)
    got = rr.evaluate(np.float32, case, sel, mutant)
    k = [s.kind for s in r64].index("neq")
    JtJ, Jtr = rr.scatter(case, r64[k].packed)
    gJ, gr = rr.scatter(case, got[k].packed.astype(np.float64))
    ok = np.linalg.norm(gr - Jtr) <= 2e-3 * np.linalg.norm(Jtr)
    B = case.B
    for a in range(case.n_frames):
        for b in range(case.n_frames):
            blk, ref = gJ[a * B:(a + 1) * B, b * B:(b + 1) * B], JtJ[a * B:(a + 1) * B, b * B:(b + 1) * B]
            ok &= np.linalg.norm(blk - ref) <= 2e-3 * np.linalg.norm(ref) + 1e-12
    return "pass (not noticed)" if ok else "fail (noticed)"
