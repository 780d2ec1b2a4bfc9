// The exact compact solve (tpc_mpc_solve_batch_compact_exact): one lane per instance runs the Newton rounds of the
// polish from U = 0 on the reference controller's model, built in registers from v (mpc_newton_compact_model.h) --
// three doubles in, two out, one launch.  Two kernel templates on the same function, so the same bits:
//   compact_exact_ws_kernel<ROWS, WARM>        run-time H (1 .. 64), per-step values in the handle's gradient workspace
//                                              ([quantity][step][instance]), as the polish keeps them
//   compact_exact_reg_kernel<HC, ROWS, WARM>   the reference's horizons 4 and 5: the horizon at compile time, every loop
//                                              over it unrolled, the per-step values in an array of the lane's own that
//                                              the compiler keeps in registers -- no workspace memory is touched
// ROWS (tpc_mpc_solve_batch_compact_exact_rows): each lane loads the ten model values of its own instance (Args::params)
// where the others read the call's from the kernel arguments.  WARM (tpc_mpc_solve_batch_compact_exact_from): the lane
// starts from its column of Args::start (one pass: load, clamp, track finiteness; a non-finite column is rewritten with
// the cold start).  Each of the twelve instantiations is a kernel of its own: the cold entries' code objects do not
// depend on the warm ones.
// The instances phase 1 could not verify are queued for the fallback (mpc_newton_fallback.h); gather-expand writes
// their general form into a compact batch for tpc_mpc_solve_batch_general and tpc_mpc_polish_batch_general, scatter
// brings the results back (the two phases: newton_two_phase, tpc_mpc_api.cpp).  Explicit fma() only
// (-ffp-contract=off): device and host path give the same bits, and both equal tpc_mpc_polish_batch_general on the
// expanded arrays.
#include "mpc_newton_compact.h"

#include <type_traits>
#include <vector>

namespace tpc {

namespace {

// What a lane does with its instance's result: the flags and its place in the fallback's queue
__device__ __forceinline__ void exact_finish(const cexact::Args& a, int64_t k, uint32_t f, uint32_t* flags) {
    const uint32_t raise = raised_flags(a.raise_not_polished, f);
    if (raise) atomicOr(flags, raise);
    fallback_enqueue(a.fb_index, a.fb_count, k, f);
}

template <bool ROWS, bool WARM>
__global__ __launch_bounds__(256) void compact_exact_ws_kernel(cexact::Args a, int H, double* ws, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    const uint32_t f = cexact::exact_instance<0, ROWS, WARM>(a, H, k, ws + k, a.n);
    exact_finish(a, k, f, flags);
}

template <int HC, bool ROWS, bool WARM>
__global__ __launch_bounds__(256) void compact_exact_reg_kernel(cexact::Args a, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.n) return;
    double regs[cexact::kSlots * HC];   // every index into it is a constant once the horizon's loops are unrolled
    const uint32_t f = cexact::exact_instance<HC, ROWS, WARM>(a, HC, k, regs, 1);
    exact_finish(a, k, f, flags);
}

// The entry a call is, as compile-time constants: f(ROWS, WARM) with ROWS = per-instance parameters given, WARM = a start
// given.  The launcher and the host path pick their instantiation through it.
template <class F>
void with_entry(const cexact::Args& a, F f) {
    using yes = std::true_type;
    using no = std::false_type;
    if (a.params) a.start ? f(yes{}, yes{}) : f(yes{}, no{});
    else a.start ? f(no{}, yes{}) : f(no{}, no{});
}

__global__ __launch_bounds__(256) void compact_exact_gather_kernel(cexact::Args a, CompactExactBatch b) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b.count) return;
    const int64_t k = b.index[j];
    // a.params != null (uniform over the launch): the rows entry, the instance's own ten values
    const grad::Model m = a.params ? cexact::build_model(cexact::instance_params<true>(a, k), a.v[k])
                                   : cexact::build_model(a, a.v[k]);
    expand_general(m, a.dy[k], a.dphi[k], 0.0, 0.0, b, j);
    for (int c = 0; c < 2 * b.H; ++c) b.controls[(int64_t)c * b.ld + j] = 0.0;
}

__global__ __launch_bounds__(256) void compact_exact_scatter_kernel(cexact::Args a, CompactExactBatch b) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b.count) return;
    const int64_t k = b.index[j], ld = b.ld;
    a.front[k] = b.u0[j];
    a.rear[k] = b.u0[ld + j];
    if (a.seq)
        for (int c = 0; c < 2 * b.H; ++c) a.seq[(int64_t)c * a.ld_seq + k] = b.controls[(int64_t)c * ld + j];
    if (a.status) a.status[k] = b.status[j];
    if (a.res_in) a.res_in[k] = b.res_in[j];
    if (a.res_out) a.res_out[k] = b.res_out[j];
    if (a.fell_back) a.fell_back[k] = 1;
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

bool compact_exact_in_registers(int H) { return H == 4 || H == 5; }

// A lane's time is its own serial chain of rounds: polish_general's block
hipError_t compact_exact(int H, const cexact::Args& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int block = rollout_grad_block(a.n);
    const unsigned grid = (unsigned)((a.n + block - 1) / block);
    with_entry(a, [&](auto rows, auto warm) {
        constexpr bool R = decltype(rows)::value, W = decltype(warm)::value;
        if (H == 4) hipLaunchKernelGGL((compact_exact_reg_kernel<4, R, W>), dim3(grid), dim3(block), 0, s, a, flags);
        else if (H == 5) hipLaunchKernelGGL((compact_exact_reg_kernel<5, R, W>), dim3(grid), dim3(block), 0, s, a, flags);
        else hipLaunchKernelGGL((compact_exact_ws_kernel<R, W>), dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    });
    return hipGetLastError();
}

// HOST arrays, on the calling thread: the same exact_instance() per instance
uint32_t compact_exact_host(int H, const cexact::Args& a) {
    std::vector<double> ws((size_t)cexact::kSlots * H);
    uint32_t flags = 0;
    with_entry(a, [&](auto rows, auto warm) {
        constexpr bool R = decltype(rows)::value, W = decltype(warm)::value;
        for (int64_t k = 0; k < a.n; ++k) {
            const uint32_t f = cexact::exact_instance<0, R, W>(a, H, k, ws.data(), 1);
            flags |= raised_flags(a.raise_not_polished, f);
        }
    });
    return flags;
}

static hipError_t batch_launch(bool scatter, const cexact::Args& a, const CompactExactBatch& b, hipStream_t s) {
    if (b.count <= 0) return hipSuccess;
    const int block = 256;
    const unsigned grid = (unsigned)((b.count + block - 1) / block);
    if (scatter) hipLaunchKernelGGL(compact_exact_scatter_kernel, dim3(grid), dim3(block), 0, s, a, b);
    else hipLaunchKernelGGL(compact_exact_gather_kernel, dim3(grid), dim3(block), 0, s, a, b);
    return hipGetLastError();
}

hipError_t compact_exact_gather(const cexact::Args& a, const CompactExactBatch& b, hipStream_t s) {
    return batch_launch(false, a, b, s);
}

hipError_t compact_exact_scatter(const cexact::Args& a, const CompactExactBatch& b, hipStream_t s) {
    return batch_launch(true, a, b, s);
}

}  // namespace tpc
