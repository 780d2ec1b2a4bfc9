// Polish of the general form (tpc_mpc_polish_batch_general): one lane per instance running every round of
// mpc_polish_model.h (polish_instance) in one launch -- a lane leaves the round loop as soon as its residual passes --
// with the per-step quantities in the handle's gradient workspace, and the same function on the calling thread for a
// host-only handle.  Argument checks and staging: tpc_mpc_api.cpp.
#include "mpc_polish_model.h"
#include "mpc_internal.h"

#include <vector>

namespace tpc {

namespace {

template <int I>
__global__ __launch_bounds__(256) void polish_kernel(polish::Args a, int H, double* ws, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t f = polish::polish_instance<I>(a, H, k, ws + k, a.n);
    if (f) atomicOr(flags, f);
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

int64_t polish_scratch_bytes(int I, int H, int64_t n) { return (int64_t)polish::slots(I) * H * n * 8; }

// DEVICE arrays; ws holds polish_scratch_bytes(I, H, n).  A lane's time is its own serial chain of rounds, as in the
// rollout's backward pass, so the block size is chosen the same way.
hipError_t polish_general(int I, int H, const polish::Args& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int block = rollout_grad_block(a.n);
    const unsigned grid = (unsigned)((a.n + block - 1) / block);
    if (I == 2)
        hipLaunchKernelGGL(polish_kernel<2>, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    else
        hipLaunchKernelGGL(polish_kernel<1>, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    return hipGetLastError();
}

// HOST arrays, on the calling thread: the same polish_instance() per instance; returns the OR of the flags
uint32_t polish_general_host(int I, int H, const polish::Args& a) {
    std::vector<double> ws((size_t)polish::slots(I) * H);
    uint32_t f = 0;
    for (int64_t k = 0; k < a.n; ++k)
        f |= I == 2 ? polish::polish_instance<2>(a, H, k, ws.data(), 1) : polish::polish_instance<1>(a, H, k, ws.data(), 1);
    return f;
}

}  // namespace tpc
