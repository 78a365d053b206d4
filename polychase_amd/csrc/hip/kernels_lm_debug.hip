// kernels_lm_debug.hip -- pc_debug_lm_decide: the product's LM decision code (pnp_lm.hpp) run on scripted sums
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "pnp_lm.hpp"

namespace pc {

constexpr int kLmSums = 56;   // PNP_ACC of kernels_tracker.hip: 45 (JtJ lower) + 9 (Jtr) + 1 (valid count) + 1 (cost)

// The decision of the device-resident LM on SCRIPTED sums (pc_debug_lm_decide): one workgroup (one wavefront) per script, the state
// in LDS like track_lm_kernel's, initialised by lm_init_state like the product's.  Per round the script's 56 sums go to LDS, the
// wavefront calls the product's own decision -- mode 0 track_consume_wave, 1 track_consume on lane 0, 2 bare lm_consume on lane 0
// (pnp_lm_reduce_consume_kernel's call) -- and the state after the round is written out.
// Rounds after `done`: modes 0 and 1 SKIP the call, as track_lm_kernel leaves its loop (`if (done) break`; track_consume has no
// test of its own and would read n_valid again); mode 2 makes the call, as the rounds enqueued past convergence do, and
// lm_consume's own test returns.  Either way a snapshot is written for every round: those after `done` repeat it.
// No spinning, no atomics, nothing grid-wide; the launcher's caller bounds n_rounds (<= 16) and the grid (<= 1024).
// A file of its own: in kernels_tracker.hip the mere presence of a second kernel with LDS of this size changes the code the compiler
// emits for track_lm_kernel (other LDS offsets, another schedule) -- a diagnostic must not move the product's instructions.
__global__ __launch_bounds__(64) void lm_decide_debug_kernel(int mode, int n_rounds, const LmConfig* __restrict__ cfgs,
                                                             const LmCamera* __restrict__ cams, const int* __restrict__ max_rounds,
                                                             const float* __restrict__ sums, LmDebugState* __restrict__ states) {
    __shared__ LmState s_state;
    __shared__ float s_out[kLmSums];
    const int tid = threadIdx.x;
    const size_t script = blockIdx.x;
    if (tid == 0) lm_init_state(s_state, cfgs[script], cams[script]);
    __syncthreads();
    for (int round = 0; round < n_rounds; round++) {
        if (tid < kLmSums) s_out[tid] = sums[(script * (size_t)n_rounds + (size_t)round) * kLmSums + tid];
        __syncthreads();
        if (mode == 2) {
            if (tid == 0) lm_consume(s_state, s_out);
        } else if (!s_state.done) {   // (uniform: read behind the barrier)
            if (mode == 0) track_consume_wave(s_state, s_out, round, max_rounds[script], tid);
            else if (tid == 0) track_consume(s_state, s_out, round, max_rounds[script]);
        }
        __syncthreads();
        if (tid == 0) lm_debug_snapshot(s_state, states + script * (size_t)n_rounds + (size_t)round);
        __syncthreads();
    }
}
void launch_lm_decide_debug(int mode, int n_scripts, int n_rounds, const LmConfig* cfgs, const LmCamera* cams, const int* max_rounds,
                            const float* sums, LmDebugState* states, hipStream_t s) {
    hipLaunchKernelGGL(lm_decide_debug_kernel, dim3(n_scripts), dim3(64), 0, s, mode, n_rounds, cfgs, cams, max_rounds, sums, states);
}

}  // namespace pc
