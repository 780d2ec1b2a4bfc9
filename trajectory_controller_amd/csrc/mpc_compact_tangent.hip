// Forward-mode derivative of the exact compact solve (tpc_mpc_solve_batch_compact_exact_forward): one lane per
// (direction, instance) pair runs the two tangent passes of the general form (three with the whole sequence) on the
// reference controller's model and its tangent, both built in registers from v, the ten values and the direction
// (mpc_compact_tangent_model.h) -- 3 + 2H doubles and the direction's values in, two doubles out.  Two kernel templates
// on the same function, so the same bits:
//   compact_tangent_ws_kernel<ROWS, WHOLE>   run-time H (1 .. 64), per-step values in the handle's gradient workspace
//                                            ([quantity][step][lane]), as the general forward keeps them
//   compact_tangent_reg_kernel<HC, ROWS>     horizons 4 and 5, row 0 only: the horizon at compile time, every loop over
//                                            it unrolled, the 4 HC per-step values in an array of the lane's own that the
//                                            compiler keeps in registers -- no workspace memory is touched
// Lane mapping as in mpc_tangent.hip: L = d * n + k.  A tangent of the shared parameters is K * 10 elements, ten per
// direction; no per-instance tangent array is read for it.
// No floating-point atomics; explicit fma() only (-ffp-contract=off): device and host path give the same bits.
#include "mpc_compact_tangent.h"

#include <type_traits>
#include <vector>

namespace tpc {

namespace {

template <bool ROWS, bool WHOLE>
__global__ __launch_bounds__(256) void compact_tangent_ws_kernel(ctan::Args a, int H, double* ws, uint32_t* flags) {
    const int64_t L = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)a.K * a.n;
    if (L >= lanes) return;
    const uint32_t f = ctan::compact_tangent_instance<0, ROWS, WHOLE>(a, H, (int)(L / a.n), L % a.n, ws + L, lanes);
    if (f) atomicOr(flags, f);
}

template <int HC, bool ROWS>
__global__ __launch_bounds__(256) void compact_tangent_reg_kernel(ctan::Args a, uint32_t* flags) {
    const int64_t L = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (int64_t)a.K * a.n;
    if (L >= lanes) return;
    double regs[ctan::slots(false) * HC];   // every index into it is a constant once the horizon's loops are unrolled
    const uint32_t f = ctan::compact_tangent_instance<HC, ROWS, false>(a, HC, (int)(L / a.n), L % a.n, regs, 1);
    if (f) atomicOr(flags, f);
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU
int64_t tangent_scratch_bytes(int I, int H, int64_t n, int K, bool whole);   // mpc_rollout_tangent.hip

bool compact_tangent_in_registers(int H, bool whole) { return !whole && (H == 4 || H == 5); }

int64_t compact_tangent_scratch_bytes(int H, int64_t n, int K, bool whole) {
    return compact_tangent_in_registers(H, whole) ? 0 : tangent_scratch_bytes(ctan::kI, H, n, K, whole);
}

// A lane's time is its own serial chain of passes over the horizon: the general forward's block
hipError_t compact_tangent(int H, const ctan::Args& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.n <= 0 || a.K <= 0) return hipSuccess;
    const int64_t lanes = (int64_t)a.K * a.n;
    const int block = rollout_grad_block(lanes);
    const unsigned grid = (unsigned)((lanes + block - 1) / block);
    const bool whole = a.tseq != nullptr;
    auto launch = [&](auto rows) {
        constexpr bool R = decltype(rows)::value;
        if (whole)
            hipLaunchKernelGGL((compact_tangent_ws_kernel<R, true>), dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
        else if (H == 4)
            hipLaunchKernelGGL((compact_tangent_reg_kernel<4, R>), dim3(grid), dim3(block), 0, s, a, flags);
        else if (H == 5)
            hipLaunchKernelGGL((compact_tangent_reg_kernel<5, R>), dim3(grid), dim3(block), 0, s, a, flags);
        else
            hipLaunchKernelGGL((compact_tangent_ws_kernel<R, false>), dim3(grid), dim3(block), 0, s, a, H, (double*)ws, flags);
    };
    if (a.params) launch(std::true_type{});
    else launch(std::false_type{});
    return hipGetLastError();
}

// HOST arrays, on the calling thread: the same compact_tangent_instance() per (direction, instance)
uint32_t compact_tangent_host(int H, const ctan::Args& a) {
    const bool whole = a.tseq != nullptr;
    std::vector<double> ws((size_t)ctan::slots(whole) * H);
    uint32_t f = 0;
    for (int d = 0; d < a.K; ++d)
        for (int64_t k = 0; k < a.n; ++k) {
            if (a.params)
                f |= whole ? ctan::compact_tangent_instance<0, true, true>(a, H, d, k, ws.data(), 1)
                           : ctan::compact_tangent_instance<0, true, false>(a, H, d, k, ws.data(), 1);
            else
                f |= whole ? ctan::compact_tangent_instance<0, false, true>(a, H, d, k, ws.data(), 1)
                           : ctan::compact_tangent_instance<0, false, false>(a, H, d, k, ws.data(), 1);
        }
    return f;
}

}  // namespace tpc
