// The step of the polished closed loop (tpc_mpc_rollout_polished): one lane per instance polishes the sequence the
// solve of this step left in the handle's working set (polish::polish_instance, every round in the lane) and, without
// leaving the lane, runs the step tail of the rollout (rollout_step_tail: plant update from the polished row 0, the
// per-step output rows, target shift).  The polish's status / residual rows of the step are written by
// polish_instance itself: the caller points them at the step's row.  Explicit fma() only (-ffp-contract=off), so the
// fused step equals tpc_mpc_polish_batch_general followed by rollout_step_kernel bit for bit.
#include "mpc_polish_model.h"
#include "mpc_rollout_step.h"

namespace tpc {

namespace {

template <int I>
__global__ __launch_bounds__(256) void rollout_polish_step_kernel(polish::Args p, RolloutStepArgs r, double* ws,
                                                                  uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.n) return;
    const uint32_t f = polish::polish_instance<I>(p, r.H, k, ws + k, p.n);
    if (f) atomicOr(flags, f);
    rollout_step_tail<double>(r, k);   // reads row 0 of the sequence this lane has just written (or left)
}

// ... with a disturbance row added to the new state (tpc_mpc_rollout_plant; r.A, r.B, r.C are the plant's, p's the
// controller's)
template <int I>
__global__ __launch_bounds__(256) void rollout_plant_polish_step_kernel(polish::Args p, RolloutStepArgs r, double* ws,
                                                                        uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.n) return;
    const uint32_t f = polish::polish_instance<I>(p, r.H, k, ws + k, p.n);
    if (f) atomicOr(flags, f);
    rollout_step_tail<double, true>(r, k);
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

// p: the polish of the working set (u = r.controls, x0 = r.x, targets = r.targets, ld = r.ld; u0 null); ws holds
// polish_scratch_bytes(I, H, n).  A lane's time is its own chain of rounds, so the block size is polish_general's.
hipError_t launch_rollout_polish_step(int I, const polish::Args& p, const RolloutStepArgs& r, void* ws, uint32_t* flags,
                                      hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    const int block = rollout_grad_block(p.n);
    const unsigned grid = (unsigned)((p.n + block - 1) / block);
    if (r.disturbance && I == 2)
        hipLaunchKernelGGL(rollout_plant_polish_step_kernel<2>, dim3(grid), dim3(block), 0, s, p, r, (double*)ws, flags);
    else if (r.disturbance)
        hipLaunchKernelGGL(rollout_plant_polish_step_kernel<1>, dim3(grid), dim3(block), 0, s, p, r, (double*)ws, flags);
    else if (I == 2)
        hipLaunchKernelGGL(rollout_polish_step_kernel<2>, dim3(grid), dim3(block), 0, s, p, r, (double*)ws, flags);
    else
        hipLaunchKernelGGL(rollout_polish_step_kernel<1>, dim3(grid), dim3(block), 0, s, p, r, (double*)ws, flags);
    return hipGetLastError();
}

}  // namespace tpc
