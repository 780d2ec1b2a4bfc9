// Backward pass of the closed loop (tpc_mpc_rollout_backward): one lane per instance running the whole reverse sweep of
// mpc_grad_model.h (rollout_instance) in one launch -- the state gradient and the parameter sums stay in registers from
// step to step, the per-step workspace of the handle is reused by every step -- and the same function on the calling
// thread for a host-only handle.  Argument checks and staging: tpc_mpc_api.cpp.
#include "mpc_grad_model.h"
#include "mpc_internal.h"

#include <vector>

namespace tpc {

namespace {

template <int I>
__global__ __launch_bounds__(256) void rollout_grad_kernel(grad::RollArgs a, int H, double* ws, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t f = grad::rollout_instance<I>(a, H, k, ws + k, a.n);
    if (f) atomicOr(flags, f);
}

// ... against a separate plant (tpc_mpc_rollout_plant_backward)
template <int I>
__global__ __launch_bounds__(256) void rollout_plant_bwd_kernel(grad::RollArgs a, grad::RollPlant pl, int H, double* ws,
                                                                uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t f = grad::rollout_instance<I, true>(a, H, k, ws + k, a.n, &pl);
    if (f) atomicOr(flags, f);
}

}  // namespace

// Block size by n.  A lane carries one instance through S x 3 passes over the horizon, so a wavefront's time is set by
// its own serial chain and the launch is fastest when the wavefronts are spread over as many CUs as possible.  256-lane
// blocks give n / 256 blocks: at 16 384 instances 64 blocks, a quarter of the MI355X's 256 CUs.  The largest of
// 256, 128, 64 that still gives at least one block per CU is used; below 64 x 256 instances every block is one
// wavefront.
int rollout_grad_block(int64_t n) {
    const int64_t kCUs = 256;
    for (int b = 256; b > 64; b /= 2)
        if ((n + b - 1) / b >= kCUs) return b;
    return 64;
}

// DEVICE arrays; ws holds grad_scratch_bytes(I, H, n) (the same per-step workspace as the single solve)
hipError_t rollout_grad(int I, int H, const grad::RollArgs& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.n <= 0 || a.steps <= 0) return hipSuccess;
    const int block = rollout_grad_block(a.n);
    const unsigned grid = (unsigned)((a.n + block - 1) / block);
    if (I == 2)
        hipLaunchKernelGGL(rollout_grad_kernel<2>, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    else
        hipLaunchKernelGGL(rollout_grad_kernel<1>, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    return hipGetLastError();
}

hipError_t rollout_plant_grad(int I, int H, const grad::RollArgs& a, const grad::RollPlant& pl, void* ws, uint32_t* flags,
                              hipStream_t s) {
    if (a.n <= 0 || a.steps <= 0) return hipSuccess;
    const int block = rollout_grad_block(a.n);
    const unsigned grid = (unsigned)((a.n + block - 1) / block);
    if (I == 2)
        hipLaunchKernelGGL(rollout_plant_bwd_kernel<2>, dim3(grid), dim3(block), 0, s, a, pl, H, (double*)ws, flags);
    else
        hipLaunchKernelGGL(rollout_plant_bwd_kernel<1>, dim3(grid), dim3(block), 0, s, a, pl, H, (double*)ws, flags);
    return hipGetLastError();
}

uint32_t rollout_plant_grad_host(int I, int H, const grad::RollArgs& a, const grad::RollPlant& pl) {
    std::vector<double> ws((size_t)grad::slots(I) * H);
    uint32_t f = 0;
    for (int64_t k = 0; k < a.n; ++k)
        f |= I == 2 ? grad::rollout_instance<2, true>(a, H, k, ws.data(), 1, &pl)
                    : grad::rollout_instance<1, true>(a, H, k, ws.data(), 1, &pl);
    return f;
}

// HOST arrays, on the calling thread: the same rollout_instance() per instance; returns the OR of the flags
uint32_t rollout_grad_host(int I, int H, const grad::RollArgs& a) {
    std::vector<double> ws((size_t)grad::slots(I) * H);
    uint32_t f = 0;
    for (int64_t k = 0; k < a.n; ++k)
        f |= I == 2 ? grad::rollout_instance<2>(a, H, k, ws.data(), 1) : grad::rollout_instance<1>(a, H, k, ws.data(), 1);
    return f;
}

}  // namespace tpc
