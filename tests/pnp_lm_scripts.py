"""Scripted sums for the decision step of the device-resident LM solver: what a residual sweep WOULD have returned, round by round,
chosen so that every branch of csrc/hip/pnp_lm.hpp's lm_advance / lm_consume and of track_consume is taken -- the CPU test
(test_pnp_lm_ref_cpu.py) runs them through the numpy restatement (pnp_lm_ref.py), the GPU test (test_pnp_lm_decision_gpu.py)
through pc_debug_lm_decide.  One set for both.

A script: dict(name, options, camera, sums float32 [ROUNDS][56], max_rounds (0 = none), tracker_only).  Lambdas are powers of
two as in test_lm_loop_cpu.py (initial 2^-10, min 2^-20, max 2^4, tolerances 2^-30) unless a case says otherwise.
`census` counts the branches from the restatement's run alone; seeds and distributions were adjusted against it, not against a GPU.
"""
import functools
import json
import os

import numpy as np

import pnp_lm_ref as ref

F = np.float32
ROUNDS = 12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIL = np.tril_indices(9)

Q0 = np.array([0.1, -0.2, 0.3, 0.9], np.float64)
Q0 = tuple(float(v) for v in (Q0 / np.linalg.norm(Q0)).astype(F))
CAMERA = dict(q_xyzw=Q0, t=(0.25, -0.5, 6.0), fx=800.0, fy=800.0, cx=320.0, cy=240.0, aspect_ratio=1.0, convention_opencv=1)
CAMERA_125 = dict(CAMERA, fx=1000.0, aspect_ratio=1.25, convention_opencv=0)


def sweep(h, g, cost, n_valid=40):
    """the 56 sums of a sweep: h 9x9 (its lower triangle is taken), g the gradient J^T r"""
    out = np.zeros(56, F)
    out[:45] = np.asarray(h, F)[TRIL]
    out[45:54] = np.asarray(g, F)
    out[54], out[55] = n_valid, cost
    return out


def script(name, rounds, options=None, camera=None, max_rounds=0, tracker_only=False):
    rounds = [np.asarray(r, F) for r in rounds]
    assert 1 <= len(rounds) <= ROUNDS, name
    rounds += [rounds[-1]] * (ROUNDS - len(rounds))   # the rounds after the script's last repeat it: they come after `done`, or reject
    return dict(name=name, options=dict(options or {}), camera=dict(camera or CAMERA), sums=np.stack(rounds), max_rounds=max_rounds,
                tracker_only=tracker_only)


def spd(rng, rows=40):
    a = rng.standard_normal((rows, 9)).astype(F)
    return (a.T @ a).astype(F)


def ill_conditioned(rng, e):
    q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
    return ((q * 10.0 ** np.linspace(0.0, -e, 9)) @ q.T).astype(F)


def expected_of(h, g, lam):
    """float64: the expected cost change of the damped step, for choosing a candidate's cost from the rho a case wants"""
    h = np.asarray(h, np.float64)
    h = np.tril(h) + np.tril(h, -1).T
    d = np.clip(np.diagonal(h), 1e-6, 1e32)
    hd = h - np.diag(np.diagonal(h)) + np.diag(d)
    step = -np.linalg.solve(hd + np.diag(d * lam), np.asarray(g, np.float64))
    return float(step @ (2 * np.asarray(g, np.float64) + hd @ step))


def descent(rng, rhos, lam0=2.0 ** -10, cost0=1024.0, n_valid=40):
    """rounds of a run in which every step is accepted with (about) the given rho"""
    lam, cost = lam0, cost0
    h, g = spd(rng), rng.standard_normal(9)
    rounds = [sweep(h, g, cost, n_valid)]
    for rho in rhos:
        cost = float(F(cost + rho * expected_of(h, g, lam)))
        f = max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
        lam = min(max(lam * f, 2.0 ** -20), 2.0 ** 4)
        h, g = spd(rng), rng.standard_normal(9)
        rounds.append(sweep(h, g, cost, n_valid))
    return rounds


# rho <= 0 on an accepted step: H = Q diag(10^linspace(0, -e, 9)) Q^T, e in [5, 8.5], g ~ N(0, 1), lambda = 2^-k, k in [14, 30) --
# the seeds of range(3000) at which the float32 restatement factorises and gets a POSITIVE expected change
RHO_SEEDS = (228, 312, 474, 570, 814, 1191, 1750, 1920, 2167, 2177, 2449, 2508, 2509, 2626, 2865, 2959)


def rho_draw(seed):
    rng = np.random.default_rng([seed, 0x1D])
    h = ill_conditioned(rng, rng.uniform(5.0, 8.5))
    return h, rng.standard_normal(9).astype(F), int(rng.integers(14, 30))


def search_rho_seeds(n=3000):
    keep = []
    for seed in range(n):
        h, g, k = rho_draw(seed)
        s = script("probe", [sweep(h, g, 8.0), sweep(h, g, 4.0)], dict(initial_lambda=2.0 ** -k, min_lambda=2.0 ** -40))
        if "rho_not_positive_finite" in ref.run_script(s, ref.BARE, _dtype()).events:
            keep.append(seed)
    return keep


def _dtype():
    from polychase_amd import hip
    return hip.LM_DEBUG_STATE_DTYPE


def pivot_matrix(off):
    h = np.eye(9, dtype=F)
    h[1, 0] = off
    return h


def named_scripts():
    out = []
    ones = np.full(9, 0.5, F)
    eye = np.eye(9, dtype=F)

    # ---- benign descent: rho near 1, lambda falls by the 1/3 floor each round until min_lambda holds it
    for seed in range(3):
        out.append(script(f"benign_descent_{seed}", descent(np.random.default_rng([seed, 1]), [0.97] * 10)))
    # ---- every candidate worse (one EQUAL): lambda 2^-10, 2^-9, 2^-7, 2^-4, 1, 16; ends at the rejection at max_lambda
    h = spd(np.random.default_rng(2))
    out.append(script("every_candidate_worse", [sweep(h, ones, c) for c in (8, 9, 8, 9, 9, 9, 9)]))
    out.append(script("every_candidate_worse_diag", [sweep(eye, ones, c) for c in (8, 9, 8, 9, 9, 9, 9)]))
    # ---- acceptance resets the growth factor: reject, accept with rho = 1/2, reject
    for seed in range(2):
        rng = np.random.default_rng([seed, 3])
        h, g = spd(rng), rng.standard_normal(9)
        accept = float(F(8.0 + 0.5 * expected_of(h, g, 2.0 ** -9)))
        out.append(script(f"acceptance_resets_growth_{seed}", [sweep(h, g, 8.0), sweep(h, g, 9.0), sweep(spd(rng), g, accept),
                                                                 sweep(h, g, accept + 1)], dict(max_iterations=3)))
    # ---- failed pivots: identity with JtJ[1][0] = 2 fails at 2^-10 .. 2^-4 and passes at lambda = 1 with a pivot of one rounding
    # error; with 8 it passes at lambda = 16 (pivot 17 - 64 / 17); with 32 it fails up to and AT max_lambda; each with max_iterations
    # reached inside the failure loop
    for off in (2.0, 8.0, 32.0):
        for mi in (100, 0, 1, 3, 4, 5, 6):
            out.append(script(f"failed_pivot_{int(off)}_max_iterations_{mi}", [sweep(pivot_matrix(off), ones, 8.0), sweep(eye, ones, 4.0),
                                                                                sweep(eye, ones, 2.0)], dict(max_iterations=mi)))
    for seed in range(6):   # a failed pivot in a later column, then success at a larger lambda; then descent
        rng = np.random.default_rng([seed, 4])
        h = spd(rng)
        k = int(rng.integers(1, 9))
        h[k, k - 1] = F(np.sqrt(float(h[k, k]) * float(h[k - 1, k - 1])) * (1.0 + 2.0 ** -(4 + seed)))
        out.append(script(f"failed_pivot_column_{k}_{seed}", [sweep(h, ones, 8.0), sweep(spd(rng), ones, 4.0), sweep(spd(rng), ones, 5.0)]))
    # ---- gradient norm below / equal to / above the tolerance, at round 0 and after an accepted step; the same for the step norm
    tol = 2.0 ** -30
    unit = np.zeros(9, F)
    held = dict(gradient_tol=0.0, initial_lambda=3.0, min_lambda=3.0, max_lambda=3.0)
    for name, gn in (("below", tol / 2), ("equal", tol), ("above", tol * 2)):
        for i in (0, 4, 8):
            g = unit.copy()
            g[i] = gn
            out.append(script(f"gradient_{name}_at_once_{i}", [sweep(eye, g, 8.0), sweep(eye, g, 4.0)], dict(step_tol=0.0)))
            out.append(script(f"gradient_{name}_after_accept_{i}", [sweep(eye, ones, 8.0), sweep(eye, g, 4.0), sweep(eye, g, 2.0)], dict(step_tol=0.0)))
            # lambda held at 3 (initial = min = max): the damped diagonal is 4, its root 2, the step -g / 4 without a rounding
            g = unit.copy()
            g[i] = gn * 4
            out.append(script(f"step_{name}_at_once_{i}", [sweep(eye, g, 8.0), sweep(eye, g, 4.0)], held))
            out.append(script(f"step_{name}_after_accept_{i}", [sweep(eye, ones, 8.0), sweep(eye, g, 4.0), sweep(eye, g, 2.0)], held))
    # ---- rho <= 0 on an accepted step (ill-conditioned, the float32 expected change positive) + the committed known-answer system
    for seed in RHO_SEEDS:
        h, g, k = rho_draw(seed)
        out.append(script(f"rho_not_positive_{seed}", [sweep(h, g, 8.0), sweep(h, g, 4.0), sweep(eye, ones, 2.0)],
                          dict(initial_lambda=2.0 ** -k, min_lambda=2.0 ** -40)))
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "llt9_ill_conditioned.json")))
    h = np.zeros((9, 9), F)
    for i, r in enumerate(d["jtj_lower_rows"]):
        h[i, :len(r)] = r
    out.append(script("golden_ill_conditioned", [sweep(h, d["jtr"], 8.0), sweep(h, d["jtr"], 4.0), sweep(eye, ones, 2.0)],
                      dict(initial_lambda=d["lambda"], min_lambda=2.0 ** -40)))
    # ---- rho near 1 (lambda at the min_lambda clamp), rho tiny, rho large; lambda above max_lambda clamped down
    for seed in range(5):
        rng = np.random.default_rng([seed, 5])
        out.append(script(f"rho_near_one_min_clamp_{seed}", descent(rng, [1.0, 0.99, 1.01]), dict(min_lambda=2.0 ** -11)))
        out.append(script(f"rho_tiny_{seed}", descent(rng, [2.0 ** -12, 1e-6, 0.02])))
        out.append(script(f"rho_large_{seed}", descent(rng, [1.5, 3.0, 0.75])))
        out.append(script(f"lambda_above_max_{seed}", descent(rng, [0.5, 0.4, 0.3], lam0=2.0 ** (5 + seed)), dict(initial_lambda=2.0 ** (5 + seed))))
    # ---- intrinsics: steps that cross each of the six bounds (the bounds equal the current value), both aspect ratios
    for cam_name, cam in (("ar1", CAMERA), ("ar125", CAMERA_125)):
        for flags_name, of, op in (("f", 1, 0), ("pp", 0, 1), ("f_pp", 1, 1)):
            for sign in (-1.0, 1.0):
                g = np.array([0.01, -0.02, 0.03, 0.1, 0.2, -0.1, 3.0 * sign, 2.0 * sign, -4.0 * sign], F)   # step ~ -g
                for bound_name, b in (("low", dict(f_low=cam["fy"], cx_low=cam["cx"], cy_low=cam["cy"])),
                                      ("high", dict(f_high=cam["fy"], cx_high=cam["cx"], cy_high=cam["cy"])),
                                      ("fx_high", dict(f_high=cam["fx"])), ("free", {})):
                    o = dict(optimize_focal_length=of, optimize_principal_point=op, **b)
                    out.append(script(f"intrinsics_{cam_name}_{flags_name}_{'up' if sign < 0 else 'down'}_{bound_name}",
                                      [sweep(eye, g, 8.0), sweep(eye, g, 4.0), sweep(eye, g, 5.0)], o, cam))
    # ---- zero rotation step: Jtr[0..2] = 0 and a block-diagonal JtJ (angle == 0 exactly); a rotation step of ~1e-20 and ~1e-23
    # (its square underflows: angle 0 or denormal)
    for seed in range(4):
        rng = np.random.default_rng([seed, 6])
        h = np.zeros((9, 9), F)
        h[:3, :3] = (lambda a: a.T @ a)(rng.standard_normal((8, 3)).astype(F))
        h[3:, 3:] = (lambda a: a.T @ a)(rng.standard_normal((12, 6)).astype(F))
        for name, rot in (("zero", 0.0), ("1e-20", 1e-20), ("1e-23", 1e-23), ("negative_zero", -0.0)):
            g = rng.standard_normal(9).astype(F)
            g[:3] = rot
            out.append(script(f"rotation_step_{name}_{seed}", [sweep(h, g, 8.0), sweep(h, g, 4.0), sweep(h, g, 2.0)]))
    # ---- non-finite sums
    rng = np.random.default_rng(7)
    h, g = spd(rng), rng.standard_normal(9).astype(F)
    for name, c in (("nan", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf)):
        out.append(script(f"candidate_cost_{name}", [sweep(h, g, 8.0), sweep(h, g, c), sweep(h, g, 4.0), sweep(h, g, 2.0)]))
        out.append(script(f"initial_cost_{name}", [sweep(h, g, c), sweep(h, g, 4.0), sweep(h, g, 2.0)]))
    for name, v in (("inf", np.inf), ("minus_inf", -np.inf), ("nan", np.nan)):
        for where, (i, j) in (("diagonal_0", (0, 0)), ("diagonal_4", (4, 4)), ("diagonal_8", (8, 8)), ("off_diagonal_10", (1, 0)), ("off_diagonal_83", (8, 3))):
            hh = h.copy()
            hh[i, j] = v
            out.append(script(f"jtj_{name}_{where}_at_once", [sweep(hh, g, 8.0), sweep(h, g, 4.0), sweep(h, g, 2.0)]))
            out.append(script(f"jtj_{name}_{where}_after_accept", [sweep(h, g, 8.0), sweep(hh, g, 4.0), sweep(h, g, 2.0)]))
        for i in (0, 5, 8):
            gg = g.copy()
            gg[i] = v
            out.append(script(f"jtr_{name}_{i}_at_once", [sweep(h, gg, 8.0), sweep(h, g, 4.0), sweep(h, g, 2.0)]))
            out.append(script(f"jtr_{name}_{i}_after_accept", [sweep(h, g, 8.0), sweep(h, gg, 4.0), sweep(h, g, 2.0)]))
    # ---- the diagonal clamp: 0, 1e-7 (below the 1e-6 floor), 1e33 (above the 1e32 cap), negative
    for name, v in (("zero", 0.0), ("1e-7", 1e-7), ("1e33", 1e33), ("negative", -3.0), ("1e-6", 1e-6), ("1e32", 1e32)):
        for i in (0, 4, 8):
            hh = np.eye(9, dtype=F)
            hh[i, i] = v
            out.append(script(f"diagonal_{name}_{i}", [sweep(hh, ones * F(1e-3), 8.0), sweep(hh, ones * F(1e-3), 4.0), sweep(eye, ones, 2.0)]))
    # ---- the tracker's rules (modes 0 and 1)
    for n in (0, 2):
        out.append(script(f"n_valid_{n}", [sweep(h, g, 8.0, n), sweep(h, g, 4.0, n)], tracker_only=True))
        out.append(script(f"n_valid_{n}_flags", [sweep(h, g, 8.0, n), sweep(h, g, 4.0, n)], dict(optimize_focal_length=1, optimize_principal_point=1), tracker_only=True))
        out.append(script(f"n_valid_{n}_then_40", [sweep(h, g, 8.0, n), sweep(h, g, 4.0, 40)], tracker_only=True))
    for cam_name, cam in (("ar1", CAMERA), ("ar125", CAMERA_125)):
        for of, op in ((0, 0), (1, 0), (0, 1), (1, 1)):
            o = dict(optimize_focal_length=of, optimize_principal_point=op)
            for n in (3, 4):
                out.append(script(f"n_valid_{n}_focal_{of}_pp_{op}_{cam_name}", [sweep(h, g, 8.0, n), sweep(h, g, 4.0 if n == 4 else 8.0, n),
                                                                              sweep(h, g, 4.0, n), sweep(h, g, 2.0, n)], o, cam, tracker_only=True))
            out.append(script(f"n_valid_3_focal_{of}_pp_{op}_{cam_name}_max_rounds_1", [sweep(h, g, 8.0, 3), sweep(h, g, 8.0, 3), sweep(h, g, 4.0, 3)],
                              o, cam, max_rounds=1, tracker_only=True))
    for mr in (1, 2, 5):
        for seed in range(2):
            out.append(script(f"round_limit_{mr}_{seed}", descent(np.random.default_rng([seed, 8]), [0.6] * 8), max_rounds=mr, tracker_only=True))
        # finishes by itself in exactly round max_rounds - 1: status stays 0
        costs = [8.0] + [4.0 / 2 ** k for k in range(mr - 1)]
        out.append(script(f"finishes_in_round_{mr}", [sweep(h, g, c) for c in costs], dict(max_iterations=mr - 1), max_rounds=mr, tracker_only=True))
        zero_g = np.zeros(9, F)
        out.append(script(f"gradient_exit_in_round_{mr}", [sweep(h, g, c) for c in costs[:-1]] + [sweep(h, zero_g, costs[-1])], max_rounds=mr, tracker_only=True))
    return out


KINDS = ("spd", "indefinite", "ill_conditioned", "non_finite")
KIND_P = (0.5, 0.15, 0.2, 0.15)
COSTS = ("lower", "equal", "higher", "non_finite")
COST_P = (0.5, 0.1, 0.3, 0.1)
RANDOM_SEEDS = 256


def random_script(seed):
    rng = np.random.default_rng([seed, 0x5C])
    cost = 64.0
    rounds = []
    for k in range(ROUNDS):
        kind = KINDS[rng.choice(4, p=KIND_P)]
        if kind == "spd":
            h = spd(rng, int(rng.integers(9, 41)))
        elif kind == "indefinite":
            h = spd(rng)
            i, j = sorted(rng.choice(9, 2, replace=False))
            h[j, i] = F(np.sqrt(float(h[i, i]) * float(h[j, j])) * rng.choice([1.0 + 2.0 ** -12, 1.001, 1.03, 1.5, -1.2]))
        elif kind == "ill_conditioned":
            h = ill_conditioned(rng, rng.uniform(3.0, 8.5)) * F(2.0 ** int(rng.integers(-4, 12)))
        else:
            h = spd(rng)
            i, j = sorted(rng.choice(9, 2))
            h[j, i] = rng.choice([np.nan, np.inf, -np.inf, 1e33, 0.0])
        g = (rng.standard_normal(9) * 2.0 ** int(rng.integers(-6, 3))).astype(F)
        if kind == "non_finite" and rng.random() < 0.3:
            g[rng.integers(9)] = rng.choice([np.nan, np.inf, -np.inf])
        c = COSTS[rng.choice(4, p=COST_P)] if k else "first"
        if c == "lower":
            cost = float(F(cost * rng.choice([0.999, 0.9, 0.5])))
            rounds.append(sweep(h, g, cost))
        elif c == "higher":
            rounds.append(sweep(h, g, float(F(cost * rng.choice([1.0 + 2.0 ** -20, 1.5])))))
        elif c == "non_finite":
            rounds.append(sweep(h, g, rng.choice([np.nan, np.inf, -np.inf])))
        else:
            rounds.append(sweep(h, g, cost))
    o = dict(max_iterations=int(rng.choice([0, 1, 2, 5, 100])), optimize_focal_length=int(rng.integers(2)), optimize_principal_point=int(rng.integers(2)),
             f_low=600.0, f_high=1100.0, cx_low=300.0, cx_high=340.0, cy_low=220.0, cy_high=260.0)
    s = script(f"random_{seed}", rounds, o, CAMERA_125 if seed % 2 else CAMERA)
    s["sums"][:, 54] = rng.choice([3, 4, 40], p=[0.1, 0.1, 0.8])
    return s


@functools.lru_cache(maxsize=None)
def all_scripts():
    return tuple(named_scripts() + [random_script(seed) for seed in range(RANDOM_SEEDS)])


@functools.lru_cache(maxsize=None)
def reference_runs(mode):
    """the restatement's run of every script, computed once per mode and shared (read-only) by the tests"""
    return tuple(ref.run_script(s, mode, _dtype()) for s in all_scripts())


def census(runs):
    """how often each branch was taken over the given runs + the number of scripts with a failed pivot followed by a success"""
    count = {b: 0 for b in ref.BRANCHES}
    count["scripts_with_success_after_failed_pivot"] = 0
    for r in runs:
        for e in r.events:
            if e in count:
                count[e] += 1
        count["scripts_with_success_after_failed_pivot"] += "success_after_failed_pivot" in r.events
    return count


# "Well-conditioned": every damped matrix a script factorises has a 2-norm condition number of at most 100 (the benign class:
# A^T A of a 40 x 9 normal matrix has ~10).  There the float32 step is the float64 one to ~n (3 n + 1) u cond ~ 1e-3 relative and the
# float64 shadow measures rounding noise of the pose; past it the shadow measures the conditioning of the script instead (over all
# finite scripts the two runs' quaternions differ by up to 2: the ill-conditioned steps are rotations by 1e8 rad).
WELL_CONDITIONED = 1e2


def is_measured(run):
    """finite and well-conditioned: the scripts on which float32 is held against the float64 shadow"""
    return run.shadow_ok and run.cond <= WELL_CONDITIONED and bool(np.all(np.isfinite(run.q64)))


def rotation_noise(runs):
    """worst |float32 restatement - float64 shadow| over the measured scripts: (a quaternion component of cam / cam_new, an entry
    of the sweep's R)"""
    q = r9 = 0.0
    for r in runs:
        if is_measured(r):
            q32 = np.stack([r.states["cam"]["q_xyzw"], r.states["cam_new"]["q_xyzw"]], axis=1).astype(np.float64)
            q = max(q, float(np.abs(q32 - r.q64).max()))
            r9 = max(r9, float(np.abs(r.states["R"].astype(np.float64) - r.R64).max()))
    return q, r9


NOISE_PROFILE = os.path.join(ROOT, "profiles", "pnp_lm_quaternion_noise.txt")


def recorded_noise():
    """(quaternion, R) as recorded in profiles/pnp_lm_quaternion_noise.txt"""
    values = dict(line.split("=") for line in open(NOISE_PROFILE).read().split() if "=" in line)
    return float(values["quaternion_noise"]), float(values["rotation_matrix_noise"])
