// The batch sum of the ten shared-parameter gradients of the compact backward passes (mpc_compact_grad.hip,
// mpc_compact_loop_grad.hip), without floating-point atomics and in an order that depends on n alone: block_partials()
// below -- a fixed butterfly over the lanes of a wavefront, the block's wavefronts in order through LDS, one partial row
// per block with plain stores -- and compact_grad_reduce() (mpc_compact_grad.hip), one block over the blocks' rows in a
// fixed order.  Every partial a call reads is one that call wrote.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tpc {

constexpr int kCompactParams = 10;   // cgrad::kParams

#if defined(__HIPCC__)
// the block's sum of every lane's row -> partials[c * gridDim.x + blockIdx.x]; every lane of the block calls it
__device__ __forceinline__ void block_partials(double (&row)[kCompactParams], double* partials) {
    constexpr int kP = kCompactParams;
    __shared__ double lds[4][kP];   // a block is at most 4 wavefronts (rollout_grad_block)
#pragma unroll
    for (int c = 0; c < kP; ++c) {
        double x = row[c];
#pragma unroll
        for (int mask = 32; mask >= 1; mask >>= 1) x = x + __shfl_xor(x, mask);   // a + b == b + a: every lane the same
        row[c] = x;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < kP; ++c) lds[wave][c] = row[c];
    __syncthreads();
    if (threadIdx.x < kP) {
        const int waves = blockDim.x >> 6;
        double x = lds[0][threadIdx.x];
        for (int w = 1; w < waves; ++w) x = x + lds[w][threadIdx.x];
        partials[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = x;
    }
}
#endif

// dparams[c] = the sum of partials[c * blocks + b] over b: one launch of compact_grad_reduce_kernel on s
hipError_t compact_grad_reduce(const double* partials, int blocks, double* dparams, hipStream_t s);

}  // namespace tpc
