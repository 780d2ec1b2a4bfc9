// Forward-mode derivative of the general form (tpc_mpc_solve_batch_general_forward): one lane per (direction, instance)
// pair running mpc_tangent_model.h (instance: the whole tangent sequence), the per-step workspace in the handle's
// device scratch, and the same function on the calling thread for a host-only handle.  Lane mapping as in
// mpc_rollout_tangent.hip.  Argument checks and staging: tpc_mpc_api.cpp.
#include "mpc_tangent_model.h"
#include "mpc_internal.h"

#include <vector>

namespace tpc {

namespace {

template <int I>
__global__ __launch_bounds__(256) void tangent_kernel(tangent::Args a, int H, double* ws, uint32_t* flags) {
    const int64_t L = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)a.K * a.n;
    if (L >= lanes) return;
    const uint32_t f = tangent::instance<I>(a, H, (int)(L / a.n), L % a.n, ws + L, lanes);
    if (f) atomicOr(flags, f);
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

// DEVICE arrays; ws holds tangent_scratch_bytes(I, H, n, K, true)
hipError_t tangent_general(int I, int H, const tangent::Args& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.n <= 0 || a.K <= 0) return hipSuccess;
    const int64_t lanes = (int64_t)a.K * a.n;
    const int block = rollout_grad_block(lanes);
    const unsigned grid = (unsigned)((lanes + block - 1) / block);
    if (I == 2)
        hipLaunchKernelGGL(tangent_kernel<2>, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    else
        hipLaunchKernelGGL(tangent_kernel<1>, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    return hipGetLastError();
}

// HOST arrays, on the calling thread: the same instance() per (direction, instance); returns the OR of the flags
uint32_t tangent_general_host(int I, int H, const tangent::Args& a) {
    std::vector<double> ws((size_t)tangent::slots(I, true) * H);
    uint32_t f = 0;
    for (int d = 0; d < a.K; ++d)
        for (int64_t k = 0; k < a.n; ++k)
            f |= I == 2 ? tangent::instance<2>(a, H, d, k, ws.data(), 1) : tangent::instance<1>(a, H, d, k, ws.data(), 1);
    return f;
}

}  // namespace tpc
