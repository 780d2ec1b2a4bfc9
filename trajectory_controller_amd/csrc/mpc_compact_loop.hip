// The compact closed loop (tpc_mpc_rollout_compact_exact): one lane per instance runs ALL steps of the Newton-first
// closed loop on the reference controller's model, built in registers from v (mpc_compact_loop_model.h) -- three
// doubles (+ x0) in, the per-step rows out, one launch; no model, target or carried sequence lives in global memory.
// Two kernels on the same function, so the same bits:
//   compact_loop_ws_kernel        run-time H (1 .. 64), the rounds' per-step values in the handle's gradient workspace
//                                 ([quantity][step][instance]); the carried controls are its working-copy slots
//   compact_loop_reg_kernel<HC>   the reference's horizons 4 and 5: the horizon at compile time, every loop over it
//                                 unrolled, the per-step values in an array of the lane's own that the compiler keeps
//                                 in registers -- the whole loop touches no workspace memory
// The instances phase 1 stopped as "not verified" are queued for the fallback (mpc_newton_fallback.h); gather-expand
// writes their general form, x0 included, into a compact batch for the polished loop, whose rows rollout_newton_move
// scatters back (the two phases: newton_two_phase, tpc_mpc_api.cpp).  Explicit fma() only (-ffp-contract=off): device
// and host path give the same bits, and both equal tpc_mpc_rollout_newton on the expanded arrays.
#include "mpc_compact_loop.h"

#include <vector>

namespace tpc {

namespace {

// What a lane does with its instance's result: first_unverified, the flags and its place in the fallback's queue
__device__ __forceinline__ void loop_finish(const cloop::Args& a, int64_t k, uint32_t f, int32_t first, uint32_t* flags) {
    if (a.first) a.first[k] = first;
    const cexact::Args& c = a.c;   // the single solve's arguments hold the queue
    const uint32_t raise = raised_flags(c.raise_not_polished, f);
    if (raise) atomicOr(flags, raise);
    fallback_enqueue(c.fb_index, c.fb_count, k, f);
}

__global__ __launch_bounds__(256) void compact_loop_ws_kernel(cloop::Args a, int H, double* ws, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.c.n) return;
    int32_t first;
    const uint32_t f = cloop::loop_instance<0>(a, H, k, ws + k, a.c.n, &first);
    loop_finish(a, k, f, first, flags);
}

template <int HC>
__global__ __launch_bounds__(256) void compact_loop_reg_kernel(cloop::Args a, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.c.n) return;
    double regs[cexact::kSlots * HC];   // every index into it is a constant once the horizon's loops are unrolled
    int32_t first;
    const uint32_t f = cloop::loop_instance<HC>(a, HC, k, regs, 1, &first);
    loop_finish(a, k, f, first, flags);
}

__global__ __launch_bounds__(256) void compact_loop_gather_kernel(cloop::Args a, CompactLoopBatch b) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b.count) return;
    const int64_t k = b.index[j];
    const grad::Model m = cexact::build_model(a.c, a.c.v[k]);
    expand_general(m, a.c.dy[k], a.c.dphi[k], a.x0 ? a.x0[k] : 0.0, a.x0 ? a.x0[a.ld_x0 + k] : 0.0, b, j);
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

bool compact_loop_in_registers(int H) { return H == 4 || H == 5; }

// A lane's time is its own serial chain of steps and rounds: polish_general's block
hipError_t compact_loop(int H, const cloop::Args& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.c.n <= 0) return hipSuccess;
    const int block = rollout_grad_block(a.c.n);
    const unsigned grid = (unsigned)((a.c.n + block - 1) / block);
    if (H == 4) hipLaunchKernelGGL(compact_loop_reg_kernel<4>, dim3(grid), dim3(block), 0, s, a, flags);
    else if (H == 5) hipLaunchKernelGGL(compact_loop_reg_kernel<5>, dim3(grid), dim3(block), 0, s, a, flags);
    else hipLaunchKernelGGL(compact_loop_ws_kernel, dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    return hipGetLastError();
}

// HOST arrays, on the calling thread: the same loop_instance() per instance
uint32_t compact_loop_host(int H, const cloop::Args& a) {
    std::vector<double> ws((size_t)cexact::kSlots * H);
    uint32_t flags = 0;
    for (int64_t k = 0; k < a.c.n; ++k) {
        int32_t first;
        const uint32_t f = cloop::loop_instance<0>(a, H, k, ws.data(), 1, &first);
        if (a.first) a.first[k] = first;
        flags |= raised_flags(a.c.raise_not_polished, f);
    }
    return flags;
}

hipError_t compact_loop_gather(const cloop::Args& a, const CompactLoopBatch& b, hipStream_t s) {
    if (b.count <= 0) return hipSuccess;
    const int block = 256;
    const unsigned grid = (unsigned)((b.count + block - 1) / block);
    hipLaunchKernelGGL(compact_loop_gather_kernel, dim3(grid), dim3(block), 0, s, a, b);
    return hipGetLastError();
}

}  // namespace tpc
