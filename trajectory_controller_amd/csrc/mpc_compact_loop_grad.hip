// Backward pass of the compact closed loop (tpc_mpc_rollout_compact_exact_backward): one lane per instance runs the
// reverse sweep over ALL steps of the loop on the reference controller's model, built in registers from v, and folds the
// chain rule of that model building in registers (mpc_compact_loop_grad_model.h) -- three doubles (+ x0), the recorded
// sequences and states and the incoming gradient in, three doubles (+ dx0 and the optional rows) out.  Two kernel
// templates on the same function, so the same bits:
//   cloop_grad_ws_kernel        run-time H (1 .. 64), one step's values in the handle's gradient workspace
//                               ([quantity][step][instance]), reused by every step of the loop
//   cloop_grad_reg_kernel<HC>   horizons 4 and 5: the horizon at compile time, every loop over it unrolled, the
//                               per-step values in an array of the lane's own that the compiler keeps in registers --
//                               no workspace memory is touched
// The gradients of the ten shared parameters are summed over the batch as the single solve's are (mpc_compact_reduce.h):
// block_partials, then compact_grad_reduce -- no floating-point atomics, every partial a call reads is one that call
// wrote.  Explicit fma() only (-ffp-contract=off): device and host path give the same per-instance bits.
#include "mpc_compact_loop_grad.h"
#include "mpc_compact_reduce.h"

#include <vector>

namespace tpc {

namespace {

constexpr int kP = cloopgrad::kParams;
static_assert(kP == kCompactParams, "block_partials (mpc_compact_reduce.h) sums rows of ten");

// partials == null: no reduction, a lane past the batch leaves at once
template <int HC>
__device__ __forceinline__ void lane_body(const cloopgrad::Args& a, int H, double* ws, int64_t wn, uint32_t* flags,
                                          double* partials) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double row[kP];
    if (k < a.n) {
        const uint32_t f = cloopgrad::loop_grad_instance<HC>(a, H, k, ws, wn, row);
        if (f) atomicOr(flags, f);
    } else {
        if (!partials) return;
#pragma unroll
        for (int c = 0; c < kP; ++c) row[c] = 0.0;
    }
    if (partials) block_partials(row, partials);   // uniform over the block
}

__global__ __launch_bounds__(256) void cloop_grad_ws_kernel(cloopgrad::Args a, int H, double* ws, uint32_t* flags,
                                                            double* partials) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    lane_body<0>(a, H, ws + (k < a.n ? k : 0), a.n, flags, partials);
}

template <int HC>
__global__ __launch_bounds__(256) void cloop_grad_reg_kernel(cloopgrad::Args a, uint32_t* flags, double* partials) {
    double regs[cloopgrad::kSlots * HC];   // every index into it is a constant once the horizon's loops are unrolled
    lane_body<HC>(a, HC, regs, 1, flags, partials);
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

bool cloop_grad_in_registers(int H) { return H == 4 || H == 5; }

int64_t cloop_grad_blocks(int64_t n) {
    const int block = rollout_grad_block(n);
    return (n + block - 1) / block;
}

int64_t cloop_grad_scratch_bytes(int H, int64_t n) {
    return cloop_grad_in_registers(H) ? 0 : (int64_t)cloopgrad::kSlots * H * n * 8;
}

// A lane's time is its own serial chain of 3 * steps passes over the horizon: the general backward's block
hipError_t cloop_grad(int H, const cloopgrad::Args& a, void* ws, double* partials, double* dparams, uint32_t* flags,
                      hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int block = rollout_grad_block(a.n);
    const unsigned grid = (unsigned)cloop_grad_blocks(a.n);
    double* part = dparams ? partials : nullptr;
    if (H == 4) hipLaunchKernelGGL(cloop_grad_reg_kernel<4>, dim3(grid), dim3(block), 0, s, a, flags, part);
    else if (H == 5) hipLaunchKernelGGL(cloop_grad_reg_kernel<5>, dim3(grid), dim3(block), 0, s, a, flags, part);
    else hipLaunchKernelGGL(cloop_grad_ws_kernel, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !dparams) return e;
    return compact_grad_reduce(part, (int)grid, dparams, s);
}

// HOST arrays, on the calling thread: the same loop_grad_instance() per instance, dparams summed in ascending k
uint32_t cloop_grad_host(int H, const cloopgrad::Args& a, double* dparams) {
    std::vector<double> ws((size_t)cloopgrad::kSlots * H);
    double sum[kP] = {0.0};
    uint32_t flags = 0;
    for (int64_t k = 0; k < a.n; ++k) {
        double row[kP];
        flags |= cloopgrad::loop_grad_instance<0>(a, H, k, ws.data(), 1, row);
        for (int c = 0; c < kP; ++c) sum[c] = sum[c] + row[c];
    }
    if (dparams)
        for (int c = 0; c < kP; ++c) dparams[c] = sum[c];
    return flags;
}

}  // namespace tpc
