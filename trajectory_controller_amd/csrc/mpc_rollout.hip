// Element-wise helpers of tpc_mpc_rollout: what the caller of dlib::mpc does between two
// operator() calls in a closed loop (reference: dlib_files/dlib/test/mpc.cpp:301-316) plus the
// target shift operator() performs itself (mpc.h:236-237).  One thread per instance, SoA,
// coalesced; HBM-bound and tiny next to the solves.  The body is rollout_step_tail (mpc_rollout_step.h), which the fused
// polish + step kernel of tpc_mpc_rollout_polished calls too.
#include "mpc_rollout_step.h"

namespace tpc {

template <typename T>
__global__ void rollout_step_kernel(RolloutStepArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    rollout_step_tail<T>(a, k);
}

// ... with a disturbance row added to the new state (tpc_mpc_rollout_plant, fp64 only)
__global__ void rollout_plant_step_kernel(RolloutStepArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    rollout_step_tail<double, true>(a, k);
}

hipError_t launch_rollout_step(int dtype, const RolloutStepArgs& a, hipStream_t s) {
    const int block = 256;
    const unsigned grid = (unsigned)((a.n + block - 1) / block);
    if (a.disturbance) hipLaunchKernelGGL(rollout_plant_step_kernel, dim3(grid), dim3(block), 0, s, a);
    else if (dtype == 0) hipLaunchKernelGGL(rollout_step_kernel<double>, dim3(grid), dim3(block), 0, s, a);
    else hipLaunchKernelGGL(rollout_step_kernel<float>, dim3(grid), dim3(block), 0, s, a);
    return hipGetLastError();
}

}  // namespace tpc
