// Backward pass of the general form (tpc_mpc_solve_batch_general_backward): one lane per instance running
// mpc_grad_model.h, the per-step workspace in the handle's device scratch, and the same function on the calling thread
// for a host-only handle.  Argument checks and staging: tpc_mpc_api.cpp.
#include "mpc_grad_model.h"
#include "mpc_internal.h"

#include <vector>

namespace tpc {

namespace {

template <int I>
__global__ __launch_bounds__(256) void grad_kernel(grad::Args a, int H, double* ws, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t f = grad::instance<I>(a, H, k, ws + k, a.n);
    if (f) atomicOr(flags, f);
}

}  // namespace

int64_t grad_scratch_bytes(int I, int H, int64_t n) { return (int64_t)grad::slots(I) * H * n * 8; }

// DEVICE arrays; ws holds grad_scratch_bytes(I, H, n)
hipError_t grad_general(int I, int H, const grad::Args& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((a.n + 255) / 256);
    if (I == 2)
        hipLaunchKernelGGL(grad_kernel<2>, dim3(grid), dim3(256), 0, s, a, H, (double*)ws, flags);
    else
        hipLaunchKernelGGL(grad_kernel<1>, dim3(grid), dim3(256), 0, s, a, H, (double*)ws, flags);
    return hipGetLastError();
}

// HOST arrays, on the calling thread: the same instance() per instance; returns the OR of the flags
uint32_t grad_general_host(int I, int H, const grad::Args& a) {
    std::vector<double> ws((size_t)grad::slots(I) * H);
    uint32_t f = 0;
    for (int64_t k = 0; k < a.n; ++k)
        f |= I == 2 ? grad::instance<2>(a, H, k, ws.data(), 1) : grad::instance<1>(a, H, k, ws.data(), 1);
    return f;
}

}  // namespace tpc
