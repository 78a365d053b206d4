"""CPU: the numpy restatement of the device solver's decision step (tests/pnp_lm_ref.py) and the scripts it is driven with
(tests/pnp_lm_scripts.py), before either is used to judge a GPU result (tests/test_pnp_lm_decision_gpu.py):
  * it reproduces the hand-derived expectations of tests/test_lm_loop_cpu.py (lambda sequences, iterations, invalid_steps, the
    exit taken) with that file's scripted answers expressed as matrices -- powers of two, every value exact, compared with ==;
  * its Cholesky factorisation and solve are core._llt9_solve's bits (the host copy the device copy is already held to);
  * the scripts reach every branch of the decision (the census), by the restatement's count alone;
  * its float64 shadow agrees with the float32 run within the forward error bound of a Cholesky solve where that bound means
    something, and the float32-vs-float64 rotation noise that bounds the GPU test is the one on record."""
import json
import os
import sys

import numpy as np
import pytest

import pnp_lm_ref as ref
import pnp_lm_scripts as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
L0, MAX, MIN, TOL = 2.0 ** -10, 2.0 ** 4, 2.0 ** -20, 2.0 ** -30
GROWING = [L0, L0 * 2, L0 * 2 * 4, L0 * 2 * 4 * 8, L0 * 2 * 4 * 8 * 16, MAX]
EYE = np.eye(9, dtype=F)
HALF = np.full(9, 0.5, F)


@pytest.fixture(scope="module")
def core():
    from polychase_amd import build
    build.build_all()
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@pytest.fixture(scope="module")
def runs():
    return S.reference_runs(ref.SERIAL)


def run(rounds, mode=ref.BARE, **options):
    return ref.run_script(S.script("case", rounds, options), mode, S._dtype())


def by_name(runs, name):
    return next(r for s, r in zip(S.all_scripts(), runs) if s["name"] == name)


def final(r, *fields):
    return tuple(r.states[f][-1].item() for f in fields)


def first(r, *fields):
    return tuple(r.states[f][0].item() for f in fields)


def lambdas(r):
    """lambda after each round, up to and including the round that finished"""
    n = int(np.argmax(r.states["done"])) + 1 if r.states["done"].any() else len(r.states)
    return [float(v) for v in r.states["lambda"][:n]]


# ---- the expectations of test_lm_loop_cpu.py ---------------------------------------------------------------------------------
def test_every_factorisation_fails():
    r = run([S.sweep(S.pivot_matrix(32.0), HALF, 8.0)])   # pivot 1 + lambda - 1024 / (1 + lambda) < 0 up to lambda = 16
    assert r.events.count("failed_pivot") == 6 and r.states["done"][0] == 1      # all six inside round 0's decision
    assert final(r, "invalid_steps", "iterations", "lambda") == (6, 5, MAX)       # the failure at MAX ends the loop (:160-162)
    assert final(r, "cost", "initial_cost", "grad_norm", "step_norm") == (8.0, 8.0, 1.5, -1.0)   # |(1/2, ..., 1/2)| = 3/2


def test_every_candidate_is_worse():
    r = run([S.sweep(EYE, HALF, c) for c in (8.0, 9.0, 8.0, 9.0, 9.0, 9.0, 9.0)])   # an equal cost is no improvement (:179)
    assert lambdas(r) == [L0] + GROWING[1:] + [MAX]
    assert int(np.argmax(r.states["done"])) == 6
    assert final(r, "invalid_steps", "iterations", "lambda", "cost") == (6, 5, MAX, 8.0)   # no iterations++ at MAX (:206-208)
    assert "failed_pivot" not in r.events and r.events.count("candidate_rejected") == 6


def test_gradient_below_tolerance_at_once():
    g = np.zeros(9, F)
    g[4] = TOL / 2
    r = run([S.sweep(EYE, g, 8.0)])
    assert r.events == ["gradient_exit"]
    assert final(r, "iterations", "invalid_steps", "step_norm", "grad_norm", "lambda", "done") == (0, 0, -1.0, TOL / 2, L0, 1)
    g[4] = TOL                                                                     # the tolerance itself is not below it (:152)
    r = run([S.sweep(EYE, g, 8.0)], step_tol=0.0)
    assert first(r, "done", "phase", "grad_norm") == (0, 1, TOL)


def test_step_below_tolerance():
    g = np.zeros(9, F)
    g[5] = 2 * TOL
    held = dict(initial_lambda=3.0, min_lambda=3.0, max_lambda=3.0, gradient_tol=0.0)   # damped diagonal 4: the step is -g / 4
    r = run([S.sweep(EYE, g, 8.0)], **held)
    assert r.events == ["step_exit"]                                               # no candidate was evaluated (:172-174)
    assert final(r, "iterations", "invalid_steps", "step_norm", "cost", "lambda", "done", "phase") == (0, 0, TOL / 2, 8.0, 3.0, 1, 0)
    g[5] = 4 * TOL
    assert first(run([S.sweep(EYE, g, 8.0)], **held), "done", "phase", "step_norm") == (0, 1, TOL)


def accepting(rho, lam=L0):
    """a candidate cost for (EYE, HALF) at cost 8 that is accepted with about the given rho"""
    return float(F(8.0 + rho * S.expected_of(EYE, HALF, lam)))


def test_acceptance_resets_the_growth_factor():
    # rejected (lambda * 2, v = 4), accepted with rho = 1/2 (lambda stays, v = 2), rejected: lambda * 2 -- not * 4.  rho is 1/2 to
    # ~1e-7, the factor 1 - (2 rho - 1)^3 is 1 to ~1e-20 and the new lambda rounds to the old one: exact
    c = accepting(0.5, 2 * L0)
    r = run([S.sweep(EYE, HALF, 8.0), S.sweep(EYE, HALF, 9.0), S.sweep(EYE, HALF, c), S.sweep(EYE, HALF, c + 1)], max_iterations=3)
    assert lambdas(r) == [L0, 2 * L0, 2 * L0, 4 * L0]
    assert final(r, "iterations", "invalid_steps", "cost", "initial_cost", "grad_norm", "v") == (3, 2, c, 8.0, 1.5, 4.0)


def test_rho_one_half_keeps_lambda_and_rho_one_divides_it_by_three():
    r = run([S.sweep(EYE, HALF, 8.0), S.sweep(EYE, HALF, accepting(0.5))], max_iterations=1)
    assert final(r, "lambda", "iterations", "invalid_steps", "done") == (L0, 1, 0, 1)
    r = run([S.sweep(EYE, HALF, 8.0), S.sweep(EYE, HALF, accepting(1.0))], max_iterations=1)   # factor = max(1/3, ~0), in double
    assert final(r, "lambda")[0] == float(F(np.float64(L0) / 3))
    r = run([S.sweep(EYE, HALF, 8.0), S.sweep(EYE, HALF, accepting(1.0))], max_iterations=1, min_lambda=L0 / 2)
    assert final(r, "lambda")[0] == L0 / 2 and "min_lambda_clamp" in r.events     # clamped to min_lambda (:195-196)


def test_expected_change_of_the_wrong_sign(runs):
    # the ill-conditioned case (:189-197): the step is accepted, lambda untouched
    for seed in S.RHO_SEEDS:
        r = by_name(runs, f"rho_not_positive_{seed}")
        assert r.events[:2] == ["rho_not_positive", "rho_not_positive_finite"] and r.solves[0]["expected"] > 0
        assert r.states["lambda"][1] == r.states["lambda"][0] and r.states["cost"][1] == 4.0 and r.states["invalid_steps"][1] == 0


def test_max_iterations_reached():
    c = [8.0]
    for _ in range(4):
        c.append(float(F(c[-1] / 2)))
    r = run([S.sweep(EYE, HALF, v) for v in c], max_iterations=4)
    assert final(r, "iterations", "cost", "invalid_steps", "done") == (4, 0.5, 0, 1) and int(np.argmax(r.states["done"])) == 4
    assert r.events.count("accepted") == 4


def test_a_failed_factorisation_takes_an_iteration_and_no_round():
    # identity with JtJ[1][0] = 2: the pivot 1 + lambda - 4 / (1 + lambda) fails at 2^-10, 2^-9, 2^-7, 2^-4 and is one rounding
    # error above zero at lambda = 1 -- all within round 0; then the candidate is accepted
    r = by_name(S.reference_runs(ref.BARE), "failed_pivot_2_max_iterations_5")
    assert [e for e in r.events if "pivot" in e] == ["failed_pivot"] * 4 + ["success_after_failed_pivot"]
    assert (r.states["lambda"][0], r.states["invalid_steps"][0], r.states["iterations"][0], r.states["phase"][0]) == (1.0, 4, 4, 1)
    assert final(r, "invalid_steps", "iterations", "done") == (4, 5, 1)
    r = by_name(S.reference_runs(ref.BARE), "failed_pivot_8_max_iterations_100")     # 17 - 64 / 17 > 0: passes at max_lambda
    assert [e for e in r.events if "pivot" in e] == ["failed_pivot"] * 5 + ["success_after_failed_pivot"]
    assert (r.states["lambda"][0], r.states["invalid_steps"][0], r.states["iterations"][0], r.states["phase"][0]) == (MAX, 5, 5, 1)
    r = by_name(S.reference_runs(ref.BARE), "failed_pivot_32_max_iterations_100")
    assert final(r, "invalid_steps", "iterations", "lambda", "done") == (6, 5, MAX, 1) and r.events.count("failed_pivot_at_max_lambda") == 1


# ---- the tracker's rules ------------------------------------------------------------------------------------------------------
def test_tracker_rules(runs):
    assert final(by_name(runs, "n_valid_2_flags"), "status", "done", "n_valid", "optimize_focal") == (1, 1, 2, 1)
    r = by_name(runs, "n_valid_3_focal_1_pp_1_ar125")
    assert (r.states["optimize_focal"][0], r.states["optimize_pp"][0], r.states["phase"][0], r.states["sweep_optimize_focal"][0]) == (0, 0, 0, 0)
    assert final(by_name(runs, "n_valid_4_focal_1_pp_1_ar125"), "optimize_focal", "optimize_pp", "status") == (1, 1, 0)
    for mr in (1, 2, 5):
        r = by_name(runs, f"round_limit_{mr}_0")
        assert list(r.states["status"]) == [0] * (mr - 1) + [3] * (S.ROUNDS - mr + 1) and r.states["done"][mr - 1] == 1
        r = by_name(runs, f"finishes_in_round_{mr}")
        assert int(np.argmax(r.states["done"])) == mr - 1 and not r.states["status"].any()
    # the rounds after `done` are not executed: every later record repeats the one that finished
    for r in runs:
        if r.states["done"].any():
            k = int(np.argmax(r.states["done"]))
            assert all(r.states[j].tobytes() == r.states[k].tobytes() for j in range(k, S.ROUNDS))


# ---- the factorisation ---------------------------------------------------------------------------------------------------------
def test_cholesky_and_solve_are_the_host_solver_bits(core):
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "llt9_ill_conditioned.json")))
    a = np.zeros((9, 9), F)
    for i, row in enumerate(d["jtj_lower_rows"]):
        a[i, :len(row)] = row
    a[np.diag_indices(9)] += F(d["lambda"])
    systems = [(a, np.array(d["jtr"], F))]
    rng = np.random.default_rng(11)
    for k in range(200):
        h = S.spd(rng, int(rng.integers(9, 41))) if k % 2 else S.ill_conditioned(rng, rng.uniform(0.0, 4.0))
        systems.append((np.tril(h), rng.standard_normal(9).astype(F)))
    for a, b in systems:
        l = a.copy()
        assert ref.cholesky9(l)
        assert ref.cholesky9_solve(l, b).tobytes() == core._llt9_solve(a, b).tobytes()
    with np.errstate(invalid="ignore"):
        assert not ref.cholesky9(-EYE.copy())
    with pytest.raises(RuntimeError):
        core._llt9_solve(-EYE, systems[0][1])


# ---- the scripts ---------------------------------------------------------------------------------------------------------------
def test_scripts_are_well_formed():
    scripts = S.all_scripts()
    assert len({s["name"] for s in scripts}) == len(scripts) <= 1024 and S.ROUNDS <= 12
    for s in scripts:
        assert s["sums"].shape == (S.ROUNDS, 56) and s["sums"].dtype == F
        assert np.all(np.isin(s["sums"][:, 54], (0, 2, 3, 4, 40))), "the valid count is converted to int on the device: finite and small"


def test_branch_census(runs):
    """every branch the issue names is taken at least 5 times over the script set, by the restatement's count"""
    count = S.census(runs)
    print("\nbranch census over", len(runs), "scripts:", count)
    for branch in ref.BRANCHES:
        assert count[branch] >= 5, branch
    assert count["scripts_with_success_after_failed_pivot"] >= 20
    # the bare decision (mode 2) runs the scripts that need no tracker rule: the same branches of lm_consume
    bare = S.census([r for s, r in zip(S.all_scripts(), S.reference_runs(ref.BARE)) if not s["tracker_only"]])
    for branch in ref.BRANCHES:
        if branch not in ("fewer_than_3", "three_drop_intrinsics", "round_limit"):
            assert bare[branch] >= 5, branch


# ---- the float64 shadow --------------------------------------------------------------------------------------------------------
def test_float64_shadow_on_the_well_conditioned_scripts(runs):
    """Cholesky solve in float32 (u = 2^-24, n = 9): backward error |dA| <= gamma_(3n+1) |L||L^T| (Higham, Accuracy and Stability
    of Numerical Algorithms, Theorem 10.4), || |L||L^T| ||_2 <= n ||A||_2, so |dx| / |x| <= n (3 n + 1) u cond / (1 - ...): twice
    that, which covers the denominator while n (3 n + 1) u cond <= 1/2.  The expected change e = s^T (2 g + H s) moves by
    de = ds^T (2 g + 2 H s) to first order plus the rounding of its own 200 operations: (bound * 2 + 32 u) |s| (|g| + |H| |s|) * 2."""
    u = 2.0 ** -24
    measured = worst_step = worst_expected = 0
    for r in runs:
        if not S.is_measured(r):
            continue
        measured += 1
        for sol in r.solves:
            bound = 2 * 9 * 28 * u * sol["cond"]
            s64 = sol["step64"]
            err = np.linalg.norm(sol["step"].astype(np.float64) - s64)
            assert err <= bound * np.linalg.norm(s64), (err, bound)
            worst_step = max(worst_step, err / (bound * np.linalg.norm(s64)))
            if "expected" in sol:
                h = np.tril(sol["jtj"]).astype(np.float64)
                scale = 2 * np.linalg.norm(s64) * (np.linalg.norm(sol["jtr"].astype(np.float64)) + np.linalg.norm(h + np.tril(h, -1).T, 2) * np.linalg.norm(s64))
                e_bound = (2 * bound + 32 * u) * scale
                e_err = abs(float(sol["expected"]) - float(sol["expected64"]))
                assert e_err <= e_bound, (e_err, e_bound)
                worst_expected = max(worst_expected, e_err / e_bound)
    print(f"\n{measured} finite well-conditioned scripts; worst error / bound: step {worst_step:.4f}, expected {worst_expected:.4f}")
    assert measured >= 100


def test_rotation_noise_is_the_one_on_record(runs):
    """profiles/pnp_lm_quaternion_noise.txt holds the worst |float32 restatement - float64 shadow| of a quaternion component and
    of an entry of R over the finite well-conditioned scripts; the GPU test allows the device 4 times what is measured here.
    numpy's float32 sin / cos may differ in the last place between machines: the record is held to a factor of 2."""
    q, r9 = S.rotation_noise(runs)
    q_rec, r9_rec = S.recorded_noise()
    print(f"\nquaternion noise {q:.4g} (recorded {q_rec:.4g}), rotation matrix noise {r9:.4g} (recorded {r9_rec:.4g})")
    assert q_rec / 2 <= q <= q_rec * 2 and r9_rec / 2 <= r9 <= r9_rec * 2
    assert 2.0 ** -24 < q < 1e-4 and 2.0 ** -24 < r9 < 1e-4   # rounding noise; a wrong term moves a component by parts in a thousand
