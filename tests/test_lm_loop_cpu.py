"""CPU: the control flow of the host solvers' one Levenberg-Marquardt loop (csrc/host/lm_loop.h, a restatement of the
reference's cpp/pnp/lev_marq.h:132-228) over a scripted problem: every operation answers from a list, so what the loop must
do follows from lev_marq.h by hand.  Every lambda is a power of two: the expected values are exact and compared with ==.
Each case runs in the scalar type of the dense solver (float) and of the banded one (double)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L0 = 2.0 ** -10            # initial_lambda
MAX = 2.0 ** 4             # max_lambda
MIN = 2.0 ** -20           # min_lambda
TOL = 2.0 ** -30           # gradient_tol and step_tol
# lambda grows by v = 2, 4, 8, ... after each failure (lev_marq.h:164-165, :210-211), saturates at MAX: 1 * 32 > 16
GROWING = [L0, L0 * 2, L0 * 2 * 4, L0 * 2 * 4 * 8, L0 * 2 * 4 * 8 * 16, MAX]
STEP = ["factorize", "solve", "evaluate"]
ACCEPT = STEP + ["expected", "accept", "report"]
REJECT = STEP + ["report"]


@pytest.fixture(scope="module")
def core():
    from polychase_amd import build
    build.build_all()
    import torch  # noqa: F401
    sys.path.insert(0, os.path.join(ROOT, "polychase_amd", "core"))
    import polychase_core
    return polychase_core


@pytest.fixture(params=["float", "double"])
def run(core, request):
    def run(costs, factorize_ok, grad_norms, step_norms, expected_changes=(), stop_at=None, max_iterations=100, min_lambda=MIN):
        o = core.BundleOptions()
        o.max_iterations = max_iterations
        o.initial_lambda, o.min_lambda, o.max_lambda = L0, min_lambda, MAX
        o.gradient_tol = o.step_tol = TOL
        return core._lm_loop_script(request.param, list(costs), list(factorize_ok), list(grad_norms), list(step_norms),
                                    list(expected_changes), stop_at, o)
    return run


def test_every_factorisation_fails(run):
    # exactly six answers: one more factorisation than expected would run the script out (an error)
    r = run([8.0], [False] * 6, [1.0], [])
    assert r["lambdas"] == GROWING
    assert (r["invalid_steps"], r["iterations"], r["lambda"]) == (6, 5, MAX)   # the failure at MAX ends the loop (:160-162)
    assert r["ops"] == ["cost", "linearize"] + ["factorize"] * 6 + ["report"]
    assert (r["cost"], r["initial_cost"], r["grad_norm"], r["step_norm"]) == (8.0, 8.0, 1.0, -1.0)


def test_every_candidate_is_worse(run):
    r = run([8.0, 9.0, 8.0, 9.0, 9.0, 9.0, 9.0], [True] * 6, [1.0], [0.5] * 6)   # an equal cost is no improvement (:179)
    assert r["lambdas"] == GROWING
    assert (r["invalid_steps"], r["iterations"], r["lambda"], r["cost"]) == (6, 5, MAX, 8.0)
    # linearised once; one evaluation per iteration; the rejection at MAX leaves without the in-loop report (:206-208)
    assert r["ops"] == ["cost", "linearize"] + REJECT * 5 + STEP + ["report"]
    assert r["reports"] == [0, 1, 2, 3, 4, 5]
    assert r["step_norm"] == 0.5


def test_gradient_below_tolerance_at_once(run):
    r = run([8.0], [], [TOL / 2], [])
    assert r["ops"] == ["cost", "linearize", "report"]
    assert (r["iterations"], r["invalid_steps"], r["step_norm"], r["grad_norm"], r["lambda"]) == (0, 0, -1.0, TOL / 2, L0)
    # the tolerance itself is not below it (:152)
    assert run([8.0], [True], [TOL], [TOL / 2])["ops"] == ["cost", "linearize", "factorize", "solve", "report"]


def test_step_below_tolerance(run):
    r = run([8.0], [True], [1.0], [TOL / 2])
    assert r["ops"] == ["cost", "linearize", "factorize", "solve", "report"]   # no candidate was evaluated (:172-174)
    assert (r["iterations"], r["invalid_steps"], r["step_norm"], r["cost"], r["lambda"]) == (0, 0, TOL / 2, 8.0, L0)


def test_acceptance_resets_the_growth_factor(run):
    # rejected (lambda * 2, v = 4), accepted with rho = 1/2 (lambda stays, v = 2), rejected: lambda * 2 -- not * 4
    r = run([8.0, 9.0, 4.0, 5.0], [True] * 3, [1.0, 0.5], [0.5] * 3, [-8.0], max_iterations=3)
    assert r["lambdas"] == [L0, 2 * L0, 2 * L0]
    assert r["lambda"] == 4 * L0
    assert r["ops"] == ["cost", "linearize"] + REJECT + ACCEPT + ["linearize"] + REJECT + ["report"]
    assert (r["iterations"], r["invalid_steps"], r["cost"], r["initial_cost"], r["grad_norm"]) == (3, 2, 4.0, 8.0, 0.5)


def test_rho_one_half_keeps_lambda(run):
    r = run([8.0, 4.0], [True], [1.0], [0.5], [-8.0], max_iterations=1)   # factor = 1 - (2 * 1/2 - 1)^3 = 1
    assert (r["lambda"], r["cost"], r["iterations"], r["invalid_steps"]) == (L0, 4.0, 1, 0)


def test_rho_one_divides_lambda_by_three(run):
    r = run([8.0, 4.0], [True], [1.0], [0.5], [-4.0], max_iterations=1)   # factor = max(1/3, 1 - 1) = 1/3, in double
    assert r["lambda"] == float(np.float32(np.float64(L0) / 3))
    r = run([8.0, 4.0], [True], [1.0], [0.5], [-4.0], max_iterations=1, min_lambda=L0 / 2)
    assert r["lambda"] == L0 / 2                                           # clamped to min_lambda (:195-196)


def test_expected_change_of_the_wrong_sign(run):
    # the ill-conditioned case (:189-197): rho = -1 would give the factor 1 - (-3)^3 = 28; the step is accepted, lambda untouched
    r = run([8.0, 4.0], [True], [1.0], [0.5], [4.0], max_iterations=1)
    assert r["ops"] == ["cost", "linearize"] + ACCEPT + ["report"]
    assert (r["lambda"], r["cost"], r["invalid_steps"]) == (L0, 4.0, 0)


def test_max_iterations_reached(run):
    r = run([32.0, 16.0, 8.0, 4.0, 2.0], [True] * 4, [1.0] * 4, [0.5] * 4, [-32.0, -16.0, -8.0, -4.0], max_iterations=4)
    assert r["ops"] == ["cost"] + (["linearize"] + ACCEPT) * 4 + ["report"]
    assert (r["iterations"], r["cost"], r["lambda"], r["invalid_steps"]) == (4, 2.0, L0, 0)
    assert r["reports"] == [0, 1, 2, 3, 4]


def test_report_stops_the_loop(run):
    r = run([32.0, 16.0, 8.0], [True] * 2, [1.0] * 2, [0.5] * 2, [-32.0, -16.0], stop_at=1)
    # stopped after iteration 1; the final report is still made, once (:216-225)
    assert r["ops"] == ["cost"] + (["linearize"] + ACCEPT) * 2 + ["report"]
    assert r["reports"] == [0, 1, 1]
    assert (r["iterations"], r["cost"]) == (1, 8.0)


def test_no_report_for_a_failed_factorisation(run):
    r = run([8.0, 4.0], [False, True], [1.0], [0.5], [-8.0], max_iterations=2)
    assert r["ops"] == ["cost", "linearize", "factorize"] + ACCEPT + ["report"]   # `continue` skips the callback (:158-169)
    assert r["reports"] == [1, 2]
    assert (r["lambdas"], r["invalid_steps"], r["iterations"]) == ([L0, 2 * L0], 1, 2)
