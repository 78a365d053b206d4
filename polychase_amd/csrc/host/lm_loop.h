// lm_loop.h -- the Levenberg-Marquardt control loop of the reference (cpp/pnp/lev_marq.h:132-228 dense, :503-601
// sparse: the same statements), once for both host solvers.  What differs between them comes from `Problem`:
//
//   using Scalar                       float (dense PnP, pnp.cc) or double (banded refiner, trajectory_refiner.cc): the type
//                                      of the cost comparison, of `actual`, `expected` and `rho`; BundleStats stays Float
//   Scalar InitialCost()               TotalCost at the start parameters                                       (:135)
//   Scalar Linearize()                 BuildNormalEquations at the accepted parameters, returns |J^T r|        (:149-151)
//   bool   Factorize(Float lambda)     ComputeStep, first half: factorise J^T J with diag * (1 + lambda), leave the clamped
//                                      diagonal in J^T J; false on a failed pivot                              (:157, :299-314)
//   Scalar Solve()                     ComputeStep, second half: step = -solve(J^T r), returns |step|          (:171)
//   Scalar EvaluateCandidate()         Step + TotalCost(params_new)                                            (:176-177)
//   Scalar ExpectedChange()            step^T (2 J^T r + J^T J step)                                           (:182-185)
//   void   Accept()                    *params = params_new                                                    (:199)
//   bool   Report(const BundleStats&)  the progress callback, false stops the loop                             (:216-225)
//
// The loop calls them in exactly that order and keeps everything else: the stats, `v`, `rebuild`, the three exits, both
// lambda-growth branches, rho and the Nielsen factor.
#pragma once

#include <algorithm>
#include <cmath>

#include "types.h"

template <class Problem>
BundleStats LevMarqLoop(const BundleOptions& opts, Problem& problem) {
    using Scalar = typename Problem::Scalar;
    BundleStats stats;
    Scalar cost = problem.InitialCost();
    stats.cost = static_cast<Float>(cost);
    stats.initial_cost = stats.cost;
    stats.grad_norm = -1;
    stats.step_norm = -1;
    stats.invalid_steps = 0;
    stats.lambda = opts.initial_lambda;

    Float v = 2.0f;
    bool rebuild = true;
    // a failed factorisation and a worse candidate (:158-168, :204-214); false: lambda is at its maximum already
    auto grow_lambda = [&] {
        stats.invalid_steps++;
        if (stats.lambda == opts.max_lambda) return false;
        stats.lambda = std::min(opts.max_lambda, stats.lambda * v);
        v = 2 * v;
        rebuild = false;
        return true;
    };
    for (stats.iterations = 0; stats.iterations < opts.max_iterations; ++stats.iterations) {
        if (rebuild) {
            stats.grad_norm = static_cast<Float>(problem.Linearize());
            if (stats.grad_norm < opts.gradient_tol) break;
        }
        if (!problem.Factorize(stats.lambda)) {
            if (!grow_lambda()) break;
            continue;
        }
        stats.step_norm = static_cast<Float>(problem.Solve());
        if (stats.step_norm < opts.step_tol) break;

        const Scalar cost_new = problem.EvaluateCandidate();
        if (cost_new < cost) {
            const Scalar actual = cost_new - cost;
            const Scalar expected = problem.ExpectedChange();
            const Scalar rho = actual / expected;
            if (rho > 0) {  // ill-conditioned JtJ can make `expected` positive (:189-197)
                const double factor = std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3));
                stats.lambda = std::clamp(static_cast<Float>(stats.lambda * factor), opts.min_lambda, opts.max_lambda);
            }
            problem.Accept();
            cost = cost_new;
            stats.cost = static_cast<Float>(cost_new);
            v = 2;
            rebuild = true;
        } else if (!grow_lambda()) {
            break;
        }
        if (!problem.Report(stats)) break;
    }
    problem.Report(stats);
    return stats;
}
