"""CPU: the float64 / float32 restatements of tests/tracker_ref.py are checked against the oracle and against finite
differences, the float32 noise the GPU bounds are made of is measured and recorded, and the bounds are shown to notice
planted errors (tests/test_pnp_sums_gpu.py and tests/test_raycast_edges_gpu.py apply them to the kernels)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_oracle as po  # noqa: E402
import tracker_ref as tr  # noqa: E402


def _record(name, lines):
    path = os.path.join(ROOT, "profiles", name)
    text = "\n".join(lines) + "\n"
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)


class _MatrixCamera(po.Camera):
    """the oracle's camera with the rotation given as the matrix the kernel gets (rounded to float32 it is no longer exactly
    orthonormal: a trip through the quaternion would change it by 6e-8)"""
    Rm = None

    def R(self):
        return self.Rm


def _oracle_camera(p):
    cam = _MatrixCamera(fx=p.fx, fy=p.fy, cx=p.cx, cy=p.cy, aspect_ratio=p.aspect_ratio, width=tr.PNP_W, height=tr.PNP_H,
                        opencv=p.opencv, t=p.t)
    cam.Rm = p.R
    return cam


@pytest.mark.parametrize("name", ["opengl-a1.0-trivial-f0-pp0", "opengl-a0.8-huber-f1-pp1", "opencv-a1.07-cauchy-f1-pp0",
                                  "opencv-a0.8-huber-f0-pp1", "size-257"])
def test_restatement_equals_the_oracle(name):
    """where the oracle is defined (weights 1, nobody behind): the same sums to 1e-12 relative"""
    c = tr.pnp_case(name, **tr.pnp_case_specs()[name])
    p = c.params
    jtj, jtr, valid, cost = tr.pnp_sums(tr.pnp_terms(np.float64, p, c.X, c.x, c.w))
    cam = _oracle_camera(p)
    JtJ, Jtr = po.normal_equations(cam, c.X.astype(np.float64), c.x.astype(np.float64), tr.LOSSES[p.loss], p.scale, p.opt_f, p.opt_pp)
    want = np.array([JtJ[a, b] for a, b in tr.TRIL])
    assert valid == c.n
    assert np.allclose(jtj, want, rtol=1e-12, atol=0)
    assert np.allclose(jtr, Jtr, rtol=1e-12, atol=1e-12 * np.abs(Jtr).max())
    assert cost == pytest.approx(po.total_cost(cam, c.X.astype(np.float64), c.x.astype(np.float64), tr.LOSSES[p.loss], p.scale), rel=1e-12)


@pytest.mark.parametrize("opencv", [False, True])
@pytest.mark.parametrize("aspect", [0.8, 1.07])
def test_jacobian_equals_central_differences(opencv, aspect):
    """all nine columns: rotation (applied on the right like QuatStepPost), translation, fy (fx = aspect * fy), cx, cy"""
    c = tr.pnp_case("fd", n=40, opencv=opencv, aspect=aspect, loss="trivial")
    p = c.params
    J = tr.pnp_terms(np.float64, p, c.X, c.x).J

    def residual(d):
        q = tr.make_params(p.R, p.t, p.fx, p.fy, p.cx, p.cy, p.aspect_ratio, p.opencv, True, True, 0, 1.0)
        w = d[:3]
        ang = np.linalg.norm(w)
        q.R = p.R @ (tr._rot(w, ang) if ang > 0 else np.eye(3))
        q.t = p.t + d[3:6]
        q.fy, q.fx = p.fy + d[6], p.fx + p.aspect_ratio * d[6]
        q.cx, q.cy = p.cx + d[7], p.cy + d[8]
        return tr.pnp_terms(np.float64, q, c.X, c.x).r

    h = 1e-6
    for k in range(9):
        d = np.zeros(9)
        d[k] = h
        fd = (residual(d) - residual(-d)) / (2 * h)
        assert np.allclose(J[:, :, k], fd, rtol=1e-6, atol=1e-6 * np.abs(J[:, :, k]).max()), k
    assert np.abs(J[:, 0, 6]).max() > 0.05           # the focal column is not small where the aspect factor shows


def test_float32_noise_of_the_sums_is_measured_and_recorded():
    """rho = max_k |sum32 - sum64| / (2^-24 A_k) over every PnP case of tests/test_pnp_sums_gpu.py; the GPU bound is 4 x the worst"""
    specs = tr.pnp_case_specs()
    rows = [(name, tr.pnp_reference(name)[3]) for name in specs]
    worst = tr.pnp_rho_worst()
    at = [max(rows, key=lambda r: r[1][k])[0] for k in range(3)]
    lines = ["float32 restatement against float64, rho = max_k |sum32 - sum64| / (2^-24 * sum_i |term_i|), tests/tracker_ref.py",
             f"cases {len(rows)}",
             f"rho_jtj  {worst[0]:.3f}  at {at[0]}", f"rho_jtr  {worst[1]:.3f}  at {at[1]}", f"rho_cost {worst[2]:.3f}  at {at[2]}",
             f"GPU bound per entry = {tr.BOUND_FACTOR:g} * rho * 2^-24 * A_k"]
    print("\n".join(lines))
    _record("tracker_pnp_sum_noise.txt", lines)
    assert all(np.isfinite(worst)) and all(w > 0 for w in worst)
    # a bound of more than 1e-2 of the absolute sum would notice nothing
    assert tr.BOUND_FACTOR * max(worst) * tr.EPS24 < 1e-2


MUTANT_CASES = {"no_aspect": "opengl-a0.8-huber-f1-pp1", "behind_sign": "opencv-a1.0-trivial-f0-pp0", "no_weight": "weights-mixed",
                "huber_r2": "opencv-a1.07-huber-f1-pp0", "d02_sign": "opengl-a1.07-cauchy-f0-pp0"}


def _breaks_the_bound(name, mutant):
    c, t64, s64, _ = tr.pnp_reference(name)
    rho = tr.pnp_rho_worst()
    got = tr.pnp_sums(tr.pnp_terms(np.float32, c.params, c.X, c.x, c.w, mutant=mutant))
    with np.errstate(invalid="ignore"):
        over = [np.abs(np.float64(got[0]) - s64[0]) > tr.BOUND_FACTOR * rho[0] * tr.EPS24 * t64.A_jtj,
                np.abs(np.float64(got[1]) - s64[1]) > tr.BOUND_FACTOR * rho[1] * tr.EPS24 * t64.A_jtr,
                np.atleast_1d(not abs(np.float64(got[3]) - s64[3]) <= tr.BOUND_FACTOR * rho[2] * tr.EPS24 * t64.A_cost)]
    return bool(np.concatenate(over).any()) or got[2] != s64[2]


@pytest.mark.parametrize("mutant", tr.MUTANTS)
def test_the_bound_rejects_a_planted_error(mutant):
    name = MUTANT_CASES[mutant]
    assert not _breaks_the_bound(name, None)
    assert _breaks_the_bound(name, mutant)


def test_moeller_trumbore_restatement_equals_the_oracle():
    sc, r64, _, _ = tr.raycast_reference("rot_scale-opengl")
    origin, dirs = tr.scene_rays(np.float64, sc)
    hit, prim, u, v, t, pos = po.raycast_closest(sc.verts, sc.tris, origin, dirs)
    assert np.array_equal(hit, r64.hit) and np.array_equal(prim[hit], r64.prim[hit])
    for a, b in ((t, r64.t), (u, r64.u), (v, r64.v), (pos, r64.pos)):        # the oracle orders its products differently
        assert np.allclose(a[hit], b[hit], rtol=1e-11, atol=1e-13)
    # equal t: the lowest index wins
    verts = np.array([[-1, -1, 2], [1, -1, 2], [0, 1, 2]], np.float32)
    r = tr.mt_closest(np.float64, verts, np.array([[0, 1, 2]] * 3), np.zeros(3), np.array([[0, 0, 1.0], [0, 0, -1.0]]))
    assert r.hit.tolist() == [True, False] and r.prim.tolist() == [0, -1] and r.t[0] == 2.0 and r.m_t[0] == 0.0


def test_ray_cast_gates_are_measured_and_few_rays_are_ambiguous():
    """delta_bary / delta_t / delta_pos between the float32 and the float64 restatement on every scene of
    tests/test_raycast_edges_gpu.py (b); the GPU gates are 4 x the worst; at most 1 % of a scene's rays may be ambiguous"""
    gates = tr.raycast_gates()
    lines = ["float32 restatement against float64 on rays where both name the same triangle, tests/tracker_ref.py",
             "scene                 delta_bary   delta_t     delta_pos   hits   ambiguous"]
    for name in tr.raycast_scene_specs():
        sc, r64, r32, d = tr.raycast_reference(name)
        amb = tr.raycast_ambiguous(r64, gates)
        lines.append(f"{name:20s}  {d[0]:.3e}  {d[1]:.3e}  {d[2]:.3e}  {int(r64.hit.sum()):5d}  {int(amb.sum()):4d} of {len(amb)}")
        assert amb.mean() <= 0.01, name
        assert r64.hit.mean() > 0.3 and (~r64.hit).mean() > 0.02, name          # hits and misses are both looked at
        # away from the ambiguous rays float32 already names the float64 triangle
        assert np.array_equal(r32.hit[~amb], r64.hit[~amb]) and np.array_equal(r32.prim[~amb], r64.prim[~amb]), name
    lines.append(f"gates = {tr.BOUND_FACTOR:g} * worst: bary {gates[0]:.3e}  t {gates[1]:.3e}  pos {gates[2]:.3e}")
    print("\n".join(lines))
    _record("tracker_raycast_gates.txt", lines)
    assert gates[0] < 1e-3 and gates[2] < 1e-3      # a gate wider than that would hide a wrong triangle's neighbour
