"""numpy restatement of the decision step of the device-resident Levenberg-Marquardt solver (csrc/hip/pnp_lm.hpp), written from
the reference's loop: LevMarqDenseSolver::Solve (cpp/pnp/lev_marq.h:132-228: the loop, BuildNormalEquations' diagonal clamp :296,
ComputeStep :299-314) and PnPProblem::Step (cpp/pnp/pnp_problem.h:101-131), turned inside out like the device code: every call of
`consume` is handed the 56 sums of ONE residual sweep ([0..44] JtJ lower triangle packed row-major, [45..53] Jtr, [54] valid count,
[55] cost) and runs the loop up to the next point where a candidate has to be evaluated.

Arithmetic: the project's float32 operation order, every operation rounded to np.float32 on its own (the library is built with
-ffp-contract=off: no fused multiply-add); the lambda factor in float64 as in lev_marq.h:193-196; np.fmax / np.fmin for the
diagonal clamp (a NaN entry becomes the floor, like cwiseMax / fmaxf).  Vector operations are only used where every element sees
the scalar code's operations in the scalar code's order.

Beside the float32 run a float64 SHADOW is carried: the control decisions (pivot test, tolerances, acceptance, lambda) are the
float32 run's, but the Cholesky factorisation, both substitutions, the expected cost change and the camera step are evaluated in
float64 on the same (float32) sums.  It is the measure for what float32 rounding does to a pose -- the one tolerance of
tests/test_pnp_lm_decision_gpu.py, where the device's sinf / cosf differ from numpy's.

The tracker's rules on top (tracker.cc:95-97, pnp_problem.h:34-35 and the round limit of the persistent launch) are `track_consume`.
"""
import numpy as np

F = np.float32
D = np.float64

WAVE, SERIAL, BARE = 0, 1, 2   # pc_debug_lm_decide's modes; the restatement has one decision: WAVE and SERIAL are the same run

OPTION_DEFAULTS = dict(max_iterations=100, initial_lambda=2.0 ** -10, min_lambda=2.0 ** -20, max_lambda=2.0 ** 4,
                       gradient_tol=2.0 ** -30, step_tol=2.0 ** -30, loss_type=0, loss_scale=1.0, optimize_focal_length=0,
                       optimize_principal_point=0, f_low=1.0, f_high=1e6, cx_low=-1e6, cx_high=1e6, cy_low=-1e6, cy_high=1e6,
                       max_inlier_error=0.0, rounds_hint=0)
CAMERA_DEFAULTS = dict(q_xyzw=(0.0, 0.0, 0.0, 1.0), t=(0.0, 0.0, 5.0), fx=800.0, fy=800.0, cx=320.0, cy=240.0, aspect_ratio=1.0,
                       convention_opencv=1)

BRANCHES = ("failed_pivot", "failed_pivot_at_max_lambda", "lambda_saturates", "growth_factor_doubles", "gradient_exit", "step_exit",
            "max_iterations_in_failure_loop", "rho_not_positive", "rho_not_positive_finite", "min_lambda_clamp", "max_lambda_clamp",
            "intrinsics_clamp", "angle_zero", "non_finite_sums", "fewer_than_3", "three_drop_intrinsics", "round_limit",
            "candidate_rejected", "rejected_at_max_lambda", "accepted")


def clamp(v, lo, hi):
    """std::clamp: v < lo ? lo : (hi < v ? hi : v) -- a NaN passes through"""
    return lo if v < lo else (hi if hi < v else v)


def cholesky9(a):
    """In-place lower Cholesky of a 9x9 array (only the lower triangle is read), left-looking: column k's entries are
    a[i][k] - sum_{j<k} a[i][j] a[k][j] with the terms subtracted in ascending j, one square root and one division per entry.
    -> False when a pivot is not positive (the entries computed after it are meaningless)."""
    ok = True
    for k in range(9):
        x = a[k, k]
        for j in range(k):
            x = x - a[k, j] * a[k, j]
        ok = ok and bool(x > 0)
        x = np.sqrt(x)
        a[k, k] = x
        if k < 8:
            s = a[k + 1:, k].copy()
            for j in range(k):
                s = s - a[k + 1:, j] * a[k, j]       # every row i > k: the same subtraction, ascending j
            a[k + 1:, k] = s / x
    return ok


def cholesky9_solve(l, b):
    """L L^T x = b: forward substitution (row i subtracts l[i][j] y[j] in ascending j), then back substitution (row i subtracts
    l[j][i] x[j] in ascending j from i + 1)"""
    y = b.copy()
    for j in range(9):
        y[j] = y[j] / l[j, j]
        if j < 8:
            y[j + 1:] = y[j + 1:] - l[j + 1:, j] * y[j]
    x = np.zeros(9, b.dtype)
    for i in range(8, -1, -1):
        s = y[i]
        for j in range(i + 1, 9):
            s = s - l[j, i] * x[j]
        x[i] = s / l[i, i]
    return x


def norm9(v):
    s = v.dtype.type(0)
    for a in range(9):
        s = s + v[a] * v[a]
    return np.sqrt(s)


def expected_change(jtj, jtr, step):
    """step^T (2 Jtr + JtJ_sym step) (lev_marq.h:182-185): row a's nine products added in ascending column, then the nine rows"""
    T = step.dtype.type
    sym = np.tril(jtj) + np.tril(jtj, -1).T
    row = np.zeros(9, step.dtype)
    for b in range(9):
        row = row + sym[:, b] * step[b]
    e = T(0)
    for a in range(9):
        e = e + step[a] * (T(2) * jtr[a] + row[a])
    return e


class Camera:
    def __init__(self, T, q, t, fx, fy, cx, cy, aspect_ratio, convention_opencv):
        self.q = np.array(q, T)
        self.t = np.array(t, T)
        self.fx, self.fy, self.cx, self.cy, self.aspect_ratio = T(fx), T(fy), T(cx), T(cy), T(aspect_ratio)
        self.convention_opencv = int(convention_opencv)

    def copy(self):
        return Camera(self.q.dtype.type, self.q, self.t, self.fx, self.fy, self.cx, self.cy, self.aspect_ratio, self.convention_opencv)

    def astype(self, T):
        return Camera(T, self.q, self.t, self.fx, self.fy, self.cx, self.cy, self.aspect_ratio, self.convention_opencv)


def step_camera(c, step, cfg, optimize_focal, optimize_pp, events=None):
    """PnPProblem::Step (pnp_problem.h:101-131): q <- q * AngleAxis(step[0..2]) (quaternion.h:11-20), t += step[3..5], the
    intrinsics stepped and clamped to their bounds"""
    T = step.dtype.type
    out = c.copy()
    angle = np.sqrt(step[0] * step[0] + step[1] * step[1] + step[2] * step[2])
    if angle > 0:
        inv = T(1) / angle
        ax, ay, az = step[0] * inv, step[1] * inv, step[2] * inv
        half = T(0.5) * angle
        s, co = np.sin(half), np.cos(half)
        bx, by, bz, bw = ax * s, ay * s, az * s, co
        qx, qy, qz, qw = c.q
        out.q[0] = qw * bx + qx * bw + qy * bz - qz * by
        out.q[1] = qw * by + qy * bw + qz * bx - qx * bz
        out.q[2] = qw * bz + qz * bw + qx * by - qy * bx
        out.q[3] = qw * bw - qx * bx - qy * by - qz * bz
    elif events is not None and angle == 0:
        events.append("angle_zero")
    out.t = c.t + step[3:6]
    lo = {k: T(F(cfg[k])) for k in ("f_low", "f_high", "cx_low", "cx_high", "cy_low", "cy_high")}
    clamped = False
    if optimize_focal:
        fy = c.fy + step[6]
        fx = fy * out.aspect_ratio
        out.fy = clamp(fy, lo["f_low"], lo["f_high"])
        out.fx = clamp(fx, lo["f_low"], lo["f_high"])
        clamped = clamped or (np.isfinite(fy) and out.fy != fy) or (np.isfinite(fx) and out.fx != fx)
    if optimize_pp:
        cx, cy = c.cx + step[7], c.cy + step[8]
        out.cx = clamp(cx, lo["cx_low"], lo["cx_high"])
        out.cy = clamp(cy, lo["cy_low"], lo["cy_high"])
        clamped = clamped or (np.isfinite(cx) and out.cx != cx) or (np.isfinite(cy) and out.cy != cy)
    if clamped and events is not None:
        events.append("intrinsics_clamp")
    return out


def rotation(c):
    """Eigen::Quaternion::toRotationMatrix, the operation order of lm_make_params"""
    T = c.q.dtype.type
    qx, qy, qz, qw = c.q
    tx, ty, tz = T(2) * qx, T(2) * qy, T(2) * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    return np.array([T(1) - (tyy + tzz), txy - twz, txz + twy, txy + twz, T(1) - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                     T(1) - (txx + tyy)], T)


class Solver:
    """The state of csrc/hip/pnp_lm.hpp's LmState, float32, with the float64 shadow of the cameras and the step"""

    def __init__(self, options, camera):
        o = dict(OPTION_DEFAULTS, **options)
        c = dict(CAMERA_DEFAULTS, **camera)
        self.cfg = o
        self.max_iterations = int(o["max_iterations"])
        self.min_lambda, self.max_lambda = F(o["min_lambda"]), F(o["max_lambda"])
        self.gradient_tol, self.step_tol = F(o["gradient_tol"]), F(o["step_tol"])
        self.optimize_focal = 1 if o["optimize_focal_length"] else 0
        self.optimize_pp = 1 if o["optimize_principal_point"] else 0
        self.cam = Camera(F, c["q_xyzw"], c["t"], c["fx"], c["fy"], c["cx"], c["cy"], c["aspect_ratio"], c["convention_opencv"])
        self.cam_new = self.cam.copy()
        self.cam64, self.cam_new64 = self.cam.astype(D), self.cam.astype(D)
        self.cur_lower, self.cur_jtr = np.zeros(45, F), np.zeros(9, F)
        self.jtj, self.diag, self.jtr, self.step = np.zeros((9, 9), F), np.zeros(9, F), np.zeros(9, F), np.zeros(9, F)
        self.step64 = np.zeros(9, D)
        self.cost = self.initial_cost = F(0)
        self.lam, self.v, self.grad_norm, self.step_norm = F(o["initial_lambda"]), F(2), F(-1), F(-1)
        self.iterations = self.invalid_steps = self.phase = self.done = self.n_valid = self.status = 0
        self.rebuild = 1
        self.set_sweep(self.cam, self.cam64)
        # what the float64 shadow is good for: False once the float32 run accepted a factorisation that float64 refuses, or
        # saw a non-finite number; cond: the largest 2-norm condition number of a damped matrix that was factorised
        self.shadow_ok, self.cond = True, 1.0
        self.solves = []     # every successful factorisation: cond, step, step64, jtj, jtr (+ expected, expected64 once accepted)
        self.events = []

    def set_sweep(self, cam, cam64):
        self.sweep, self.sweep64 = cam.copy(), cam64.copy()
        self.sweep_flags = (self.optimize_focal, self.optimize_pp)
        self.R, self.R64 = rotation(cam), rotation(cam64)

    def finish(self):
        self.done = 1
        self.set_sweep(self.cam, self.cam64)

    def advance(self):
        """the top of the loop (lev_marq.h:146-176) until a candidate has to be evaluated"""
        failed_before = False
        while self.iterations < self.max_iterations:
            if self.rebuild:
                self.jtj[np.tril_indices(9)] = self.cur_lower
                self.jtr = self.cur_jtr.copy()
                self.diag = np.fmin(np.fmax(np.diagonal(self.jtj).copy(), F(1e-6)), F(1e32))   # (:296)
                self.grad_norm = norm9(self.jtr)
                if self.grad_norm < self.gradient_tol:
                    self.events.append("gradient_exit")
                    break
            # ComputeStep (:299-314)
            l = np.tril(self.jtj)
            damped = self.diag * (F(1) + self.lam)
            l[np.diag_indices(9)] = damped
            self.jtj[np.diag_indices(9)] = self.diag    # "remove dampening" leaves the clamped diagonal
            l64 = l.astype(D)
            l64[np.diag_indices(9)] = self.diag.astype(D) * (D(1) + D(self.lam))
            sym64 = np.tril(l64) + np.tril(l64, -1).T
            if not cholesky9(l):
                self.invalid_steps += 1
                self.events.append("failed_pivot")
                failed_before = True
                if self.lam == self.max_lambda:
                    self.events.append("failed_pivot_at_max_lambda")
                    break
                self.grow_lambda()
                self.rebuild = 0
                self.iterations += 1
                if not self.iterations < self.max_iterations:
                    self.events.append("max_iterations_in_failure_loop")
                continue
            if failed_before:
                self.events.append("success_after_failed_pivot")
            self.step = -cholesky9_solve(l, self.jtr)
            cond = float(np.linalg.cond(sym64)) if np.all(np.isfinite(sym64)) else np.inf
            self.cond = max(self.cond, cond)
            if cholesky9(l64):
                self.step64 = -cholesky9_solve(l64, self.jtr.astype(D))
            else:
                self.shadow_ok = False
            self.solves.append(dict(cond=cond, step=self.step.copy(), step64=self.step64.copy(), jtj=self.jtj.copy(), jtr=self.jtr.copy()))
            self.step_norm = norm9(self.step)
            if self.step_norm < self.step_tol:
                self.events.append("step_exit")
                break
            self.cam_new = step_camera(self.cam, self.step, self.cfg, self.optimize_focal, self.optimize_pp, self.events)
            self.cam_new64 = step_camera(self.cam64, self.step64, self.cfg, self.optimize_focal, self.optimize_pp)
            self.set_sweep(self.cam_new, self.cam_new64)
            self.phase = 1
            return
        self.finish()

    def grow_lambda(self):
        if self.v > 2:
            self.events.append("growth_factor_doubles")
        grown = self.lam * self.v
        self.lam = np.fmin(self.max_lambda, grown)
        if grown >= self.max_lambda:
            self.events.append("lambda_saturates")
        self.v = F(2) * self.v

    def consume(self, sums):
        """lm_consume: one sweep's sums -> the next parameters to evaluate, or done"""
        if self.done:
            return
        if not np.all(np.isfinite(sums)):
            self.events.append("non_finite_sums")
            self.shadow_ok = False
        if self.phase == 0:    # the initial parameters (:134-145)
            self.cur_lower, self.cur_jtr = sums[:45].copy(), sums[45:54].copy()
            self.cost = self.initial_cost = sums[55]
            self.rebuild = 1
            self.advance()
            return
        cost_new = sums[55]
        if cost_new < self.cost:
            actual = cost_new - self.cost
            expected = expected_change(self.jtj, self.jtr, self.step)
            self.solves[-1].update(expected=expected, expected64=expected_change(self.jtj.astype(D), self.jtr.astype(D), self.step64))
            rho = actual / expected
            if rho > 0:     # (:189-197)
                d = 2.0 * float(rho) - 1.0
                f = 1.0 - d * d * d
                factor = f if f > 1.0 / 3.0 else 1.0 / 3.0
                scaled = F(float(self.lam) * factor)
                self.lam = clamp(scaled, self.min_lambda, self.max_lambda)
                if scaled < self.min_lambda:
                    self.events.append("min_lambda_clamp")
                elif self.max_lambda < scaled:
                    self.events.append("max_lambda_clamp")
            else:
                self.events.append("rho_not_positive")
                if np.isfinite(actual) and np.isfinite(expected) and expected != 0:
                    self.events.append("rho_not_positive_finite")
            self.events.append("accepted")
            self.cam, self.cam64 = self.cam_new.copy(), self.cam_new64.copy()
            self.cur_lower, self.cur_jtr = sums[:45].copy(), sums[45:54].copy()
            self.cost = cost_new
            self.v = F(2)
            self.rebuild = 1
        else:
            self.invalid_steps += 1
            self.events.append("candidate_rejected")
            if self.lam == self.max_lambda:
                self.events.append("rejected_at_max_lambda")
                self.finish()
                return
            self.grow_lambda()
            self.rebuild = 0
        self.iterations += 1
        self.advance()

    def track_consume(self, sums, round_, max_rounds):
        """the tracker's rules around the decision (kernels_tracker.hip: track_consume)"""
        if self.phase == 0:
            self.n_valid = int(sums[54])
            if self.n_valid < 3:       # "Not enough features" (tracker.cc:95-97)
                self.status = 1
                self.events.append("fewer_than_3")
                self.finish()
                return
            if self.n_valid == 3 and (self.optimize_focal or self.optimize_pp):
                # intrinsics are only optimised with more than 3 points (pnp_problem.h:34-35): the round is repeated without
                self.optimize_focal = self.optimize_pp = 0
                self.events.append("three_drop_intrinsics")
                self.set_sweep(self.cam, self.cam64)
                return
        self.consume(sums)
        if not self.done and round_ + 1 >= max_rounds:
            self.status = 3
            self.events.append("round_limit")
            self.finish()

    def snapshot(self):
        def cam(c):
            return (c.q.copy(), c.t.copy(), c.fx, c.fy, c.cx, c.cy, c.aspect_ratio, c.convention_opencv)
        s = self.sweep
        return (cam(self.cam), cam(self.cam_new), self.R.copy(), s.t.copy(), s.fx, s.fy, s.cx, s.cy, s.aspect_ratio,
                s.convention_opencv, self.sweep_flags[0], self.sweep_flags[1], self.jtj.reshape(81).copy(), self.diag.copy(),
                self.jtr.copy(), self.step.copy(), self.cost, self.initial_cost, self.lam, self.v, self.grad_norm, self.step_norm,
                self.iterations, self.invalid_steps, self.rebuild, self.phase, self.done, self.n_valid, self.status,
                self.optimize_focal, self.optimize_pp)


class Run:
    """What a script did: states (one record of `dtype` per round, float32), the float64 shadow of the rotations per round
    (q64 [rounds][2][4] of cam / cam_new, R64 [rounds][9]), the branches taken (events), every successful factorisation with both
    steps (solves), and what the shadow is worth: shadow_ok, cond = the largest condition number of a factorised damped matrix."""


def run_script(script, mode, dtype):
    """script: dict(options, camera, sums float32 [rounds][56], max_rounds) -> Run.  mode BARE: the decision alone, every round
    handed to `consume`; otherwise the tracker's rules, and the rounds after `done` are not executed (their records repeat)."""
    sums = np.ascontiguousarray(script["sums"], F)
    max_rounds = script.get("max_rounds") or (1 << 30)
    r = Run()
    r.states = np.zeros(len(sums), dtype)
    r.q64, r.R64 = np.zeros((len(sums), 2, 4)), np.zeros((len(sums), 9))
    with np.errstate(all="ignore"):
        s = Solver(script.get("options", {}), script.get("camera", {}))
        for k in range(len(sums)):
            if mode == BARE:
                s.consume(sums[k])
            elif not s.done:
                s.track_consume(sums[k], k, max_rounds)
            r.states[k] = s.snapshot()
            r.q64[k, 0], r.q64[k, 1], r.R64[k] = s.cam64.q, s.cam_new64.q, s.R64
    r.events, r.shadow_ok, r.cond, r.solves = s.events, s.shadow_ok, s.cond, s.solves
    return r
