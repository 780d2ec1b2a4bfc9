// Backward pass of the exact compact solve (tpc_mpc_solve_batch_compact_exact_backward): one lane per instance runs the
// adjoint sweep of the general form on the reference controller's model, built in registers from v, and folds the
// chain rule of that model building in registers (mpc_compact_grad_model.h) -- 3 + 2H doubles and the incoming gradient
// in, three doubles out.  Two kernel templates on the same function, so the same bits:
//   compact_grad_ws_kernel<ROWS>        run-time H (1 .. 64), per-step values in the handle's gradient workspace
//                                       ([quantity][step][instance]), as the general backward keeps them
//   compact_grad_reg_kernel<HC, ROWS>   horizons 4 and 5: the horizon at compile time, every loop over it unrolled, the
//                                       per-step values in an array of the lane's own that the compiler keeps in
//                                       registers -- no workspace memory is touched
// The gradients of the ten shared parameters are summed over the batch without floating-point atomics, in an order that
// depends on n alone: a fixed butterfly over the lanes of a wavefront, the block's wavefronts in order through LDS, one
// partial row per block with plain stores (block_partials, mpc_compact_reduce.h: shared with the compact closed loop's
// backward pass), and compact_grad_reduce_kernel (one block) over the blocks in a fixed order.
// Every partial a call reads is one that call wrote.  Explicit fma() only (-ffp-contract=off): device and host path give
// the same per-instance bits.
#include "mpc_compact_grad.h"
#include "mpc_compact_reduce.h"

#include <type_traits>
#include <vector>

namespace tpc {

namespace {

constexpr int kP = cgrad::kParams;
constexpr int kReduceBlock = 256;

static_assert(kP == kCompactParams, "block_partials (mpc_compact_reduce.h) sums rows of cgrad::kParams");

// partials == null: no reduction, a lane past the batch leaves at once
template <int HC, bool ROWS = false>
__device__ __forceinline__ void lane_body(const cgrad::Args& a, int H, double* ws, int64_t wn, uint32_t* flags,
                                          double* partials) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double row[kP];
    if (k < a.n) {
        const uint32_t f = cgrad::compact_grad_instance<HC, ROWS>(a, H, k, ws, wn, row);
        if (f) atomicOr(flags, f);
    } else {
        if (!partials) return;
#pragma unroll
        for (int c = 0; c < kP; ++c) row[c] = 0.0;
    }
    if (partials) block_partials(row, partials);   // uniform over the block
}

// ROWS (tpc_mpc_solve_batch_compact_exact_rows_backward): the lane loads its instance's ten model values from a.params,
// and its row is the gradient with respect to them
template <bool ROWS>
__global__ __launch_bounds__(256) void compact_grad_ws_kernel(cgrad::Args a, int H, double* ws, uint32_t* flags,
                                                              double* partials) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    lane_body<0, ROWS>(a, H, ws + (k < a.n ? k : 0), a.n, flags, partials);
}

template <int HC, bool ROWS>
__global__ __launch_bounds__(256) void compact_grad_reg_kernel(cgrad::Args a, uint32_t* flags, double* partials) {
    double regs[cgrad::kSlots * HC];   // every index into it is a constant once the horizon's loops are unrolled
    lane_body<HC, ROWS>(a, HC, regs, 1, flags, partials);
}

// one block: dparams[c] = the sum of partials[c * blocks + b] over b, in an order that depends on `blocks` alone
__global__ __launch_bounds__(kReduceBlock) void compact_grad_reduce_kernel(const double* partials, int blocks,
                                                                           double* dparams) {
    __shared__ double lds[kReduceBlock];
    const int tid = threadIdx.x;
    for (int c = 0; c < kP; ++c) {
        double x = 0.0;
        for (int b = tid; b < blocks; b += kReduceBlock) x = x + partials[(int64_t)c * blocks + b];
        lds[tid] = x;
        __syncthreads();
        for (int half = kReduceBlock / 2; half > 0; half >>= 1) {
            if (tid < half) lds[tid] = lds[tid] + lds[tid + half];
            __syncthreads();
        }
        if (tid == 0) dparams[c] = lds[0];
        __syncthreads();
    }
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

bool compact_grad_in_registers(int H) { return H == 4 || H == 5; }

int64_t compact_grad_blocks(int64_t n) {
    const int block = rollout_grad_block(n);
    return (n + block - 1) / block;
}

int64_t compact_grad_scratch_bytes(int H, int64_t n) {
    return compact_grad_in_registers(H) ? 0 : (int64_t)cgrad::kSlots * H * n * 8;
}

// A lane's time is its own serial chain of three passes over the horizon: the general backward's block
hipError_t compact_grad(int H, const cgrad::Args& a, void* ws, double* partials, double* dparams, uint32_t* flags,
                        hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int block = rollout_grad_block(a.n);
    const unsigned grid = (unsigned)compact_grad_blocks(a.n);
    double* part = dparams ? partials : nullptr;
    auto launch = [&](auto rows) {
        constexpr bool R = decltype(rows)::value;
        if (H == 4) hipLaunchKernelGGL((compact_grad_reg_kernel<4, R>), dim3(grid), dim3(block), 0, s, a, flags, part);
        else if (H == 5) hipLaunchKernelGGL((compact_grad_reg_kernel<5, R>), dim3(grid), dim3(block), 0, s, a, flags, part);
        else hipLaunchKernelGGL((compact_grad_ws_kernel<R>), dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags, part);
    };
    if (a.params) launch(std::true_type{});
    else launch(std::false_type{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !dparams) return e;
    return compact_grad_reduce(part, (int)grid, dparams, s);
}

hipError_t compact_grad_reduce(const double* partials, int blocks, double* dparams, hipStream_t s) {
    hipLaunchKernelGGL(compact_grad_reduce_kernel, dim3(1), dim3(kReduceBlock), 0, s, partials, blocks, dparams);
    return hipGetLastError();
}

// HOST arrays, on the calling thread: the same compact_grad_instance() per instance, dparams summed in ascending k
uint32_t compact_grad_host(int H, const cgrad::Args& a, double* dparams) {
    std::vector<double> ws((size_t)cgrad::kSlots * H);
    double sum[kP] = {0.0};
    uint32_t flags = 0;
    for (int64_t k = 0; k < a.n; ++k) {
        double row[kP];
        flags |= a.params ? cgrad::compact_grad_instance<0, true>(a, H, k, ws.data(), 1, row)
                          : cgrad::compact_grad_instance<0>(a, H, k, ws.data(), 1, row);
        for (int c = 0; c < kP; ++c) sum[c] = sum[c] + row[c];
    }
    if (dparams)
        for (int c = 0; c < kP; ++c) dparams[c] = sum[c];
    return flags;
}

}  // namespace tpc
