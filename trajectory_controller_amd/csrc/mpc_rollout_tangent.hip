// Forward-mode derivative of the closed loop (tpc_mpc_rollout_forward): one lane per (direction, instance) pair running
// the whole sweep of mpc_tangent_model.h (rollout_instance) in one launch -- the state tangent stays in registers from
// step to step, the lane's per-step workspace is reused by every step -- and the same function on the calling thread
// for a host-only handle.  Lane L is direction L / n of instance L % n, so the 64 lanes of a wavefront read 64
// consecutive instances of one direction's arrays (a wavefront that straddles two directions reads two such runs).
// Argument checks and staging: tpc_mpc_api.cpp.
#include "mpc_tangent_model.h"
#include "mpc_internal.h"

#include <vector>

namespace tpc {

namespace {

template <int I>
__global__ __launch_bounds__(256) void rollout_tangent_kernel(tangent::RollArgs a, int H, double* ws, uint32_t* flags) {
    const int64_t L = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)a.K * a.n;
    if (L >= lanes) return;
    const uint32_t f = tangent::rollout_instance<I>(a, H, (int)(L / a.n), L % a.n, ws + L, lanes);
    if (f) atomicOr(flags, f);
}

// ... against a separate plant (tpc_mpc_rollout_plant_forward)
template <int I>
__global__ __launch_bounds__(256) void rollout_plant_fwd_kernel(tangent::RollArgs a, tangent::RollPlant pl, int H,
                                                                double* ws, uint32_t* flags) {
    const int64_t L = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)a.K * a.n;
    if (L >= lanes) return;
    const uint32_t f = tangent::rollout_instance<I, true>(a, H, (int)(L / a.n), L % a.n, ws + L, lanes, &pl);
    if (f) atomicOr(flags, f);
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

// the per-step workspace of K directions of n instances: [quantity][step][lane]
int64_t tangent_scratch_bytes(int I, int H, int64_t n, int K, bool whole) {
    return (int64_t)tangent::slots(I, whole) * H * n * K * 8;
}

// DEVICE arrays; ws holds tangent_scratch_bytes(I, H, n, K, false)
hipError_t rollout_tangent(int I, int H, const tangent::RollArgs& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.n <= 0 || a.steps <= 0 || a.K <= 0) return hipSuccess;
    const int64_t lanes = (int64_t)a.K * a.n;
    const int block = rollout_grad_block(lanes);
    const unsigned grid = (unsigned)((lanes + block - 1) / block);
    if (I == 2)
        hipLaunchKernelGGL(rollout_tangent_kernel<2>, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    else
        hipLaunchKernelGGL(rollout_tangent_kernel<1>, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    return hipGetLastError();
}

hipError_t rollout_plant_tangent(int I, int H, const tangent::RollArgs& a, const tangent::RollPlant& pl, void* ws,
                                 uint32_t* flags, hipStream_t s) {
    if (a.n <= 0 || a.steps <= 0 || a.K <= 0) return hipSuccess;
    const int64_t lanes = (int64_t)a.K * a.n;
    const int block = rollout_grad_block(lanes);
    const unsigned grid = (unsigned)((lanes + block - 1) / block);
    if (I == 2)
        hipLaunchKernelGGL(rollout_plant_fwd_kernel<2>, dim3(grid), dim3(block), 0, s, a, pl, H, (double*)ws, flags);
    else
        hipLaunchKernelGGL(rollout_plant_fwd_kernel<1>, dim3(grid), dim3(block), 0, s, a, pl, H, (double*)ws, flags);
    return hipGetLastError();
}

uint32_t rollout_plant_tangent_host(int I, int H, const tangent::RollArgs& a, const tangent::RollPlant& pl) {
    std::vector<double> ws((size_t)tangent::slots(I, false) * H);
    uint32_t f = 0;
    for (int d = 0; d < a.K; ++d)
        for (int64_t k = 0; k < a.n; ++k)
            f |= I == 2 ? tangent::rollout_instance<2, true>(a, H, d, k, ws.data(), 1, &pl)
                        : tangent::rollout_instance<1, true>(a, H, d, k, ws.data(), 1, &pl);
    return f;
}

// HOST arrays, on the calling thread: the same rollout_instance() per (direction, instance); returns the OR of the flags
uint32_t rollout_tangent_host(int I, int H, const tangent::RollArgs& a) {
    std::vector<double> ws((size_t)tangent::slots(I, false) * H);
    uint32_t f = 0;
    for (int d = 0; d < a.K; ++d)
        for (int64_t k = 0; k < a.n; ++k)
            f |= I == 2 ? tangent::rollout_instance<2>(a, H, d, k, ws.data(), 1)
                        : tangent::rollout_instance<1>(a, H, d, k, ws.data(), 1);
    return f;
}

}  // namespace tpc
