// The Newton-first closed loop (tpc_mpc_rollout_newton): one lane per instance runs ALL steps of the polished closed
// loop without a first-order solve -- per step dlib's shift of the carried controls (mpc.h:231-232), the polish from
// that shifted sequence (polish::polish_instance, unchanged) and, when the polish verifies, the step tail of the
// rollout (rollout_step_tail) -- and leaves the step loop at the first step the polish cannot verify.  The per-step
// quantities of the polish live in the handle's gradient workspace ([quantity][step][instance]); nothing private is
// indexed by the horizon step.  The shift is done in the working set's control array, in place: it is what
// polish_instance reads its start from (its working copy in the workspace is rebuilt from it at every call).
// Explicit fma() only (-ffp-contract=off), so a verified step equals tpc_mpc_polish_batch_general on the shifted
// sequence followed by rollout_step_kernel bit for bit, on the device and on the host path below.
// The instances that stopped with "not polished" are queued for the fallback (mpc_newton_fallback.h); two small kernels
// move their rows into and out of the compact batch that tpc_mpc_rollout_polished's loop then runs.  How the two phases
// fit together is said once, at newton_two_phase (tpc_mpc_api.cpp).
#include "mpc_rollout_newton.h"
#include "mpc_newton_fallback.h"
#include "mpc_rollout_step.h"

#include <vector>

namespace tpc {

namespace {

using polish::per_step;

// One instance, every step.  Returns the flags of the step it stopped at (0: verified at every step) and that step in
// *first.  Rows of the per-step outputs from *first on are cleared: status -1, everything else 0, and so is the
// carried sequence.  With Plant (tpc_mpc_rollout_plant) the tail keeps the arrays a.r names -- the plant's, or the
// controller's again where the caller gave none -- and adds the disturbance's row; a non-finite plant or disturbance
// value stops the instance at step 0 with TPC_MPC_FLAG_NONFINITE, as a non-finite model does.
template <int I, bool Plant = false>
TPC_GRAD_HD uint32_t newton_instance(const NewtonArgs& a, int64_t k, double* ws0, int64_t wn, int32_t* first) {
    double* ws = ws0;
    polish::Args p = a.p;
    RolloutStepArgs r = a.r;
    // one working set (mpc_rollout_newton.h): naming it once keeps a single copy of these in scalar registers
    r.n = p.n; r.ld = p.ld; r.I = I;
    if (!Plant) { r.A = p.A; r.B = p.B; r.C = p.C; }
    r.x = const_cast<double*>(p.x0); r.targets = const_cast<double*>(p.targets); r.controls = p.u;
    const int H = r.H, S = r.steps;
    const int64_t ld = p.ld, lo = r.ld_out, k0 = k;
    uint32_t f = 0;
    int st = 0;
    if (Plant) {   // a non-finite plant or disturbance value makes the state non-finite: step 0's polish then stops the
                   // instance with TPC_MPC_FLAG_NONFINITE, and nothing has to be remembered across the steps
        bool plant_fin = true;
        const double *A = (const double*)r.A + k, *B = (const double*)r.B + k, *Cc = (const double*)r.C + k;
        for (int c = 0; c < 4; ++c) plant_fin = plant_fin && grad::gfinite(A[(int64_t)c * ld]);
        for (int c = 0; c < 2 * I; ++c) plant_fin = plant_fin && grad::gfinite(B[(int64_t)c * ld]);
        for (int c = 0; c < 2; ++c) plant_fin = plant_fin && grad::gfinite(Cc[(int64_t)c * ld]);
        if (r.disturbance)
            for (int64_t c = 0; c < 2 * (int64_t)S; ++c)
                plant_fin = plant_fin && grad::gfinite(((const double*)r.disturbance)[c * r.ld_d + k]);
        if (!plant_fin) ((double*)r.x)[k] = __builtin_nan("");
    }
    for (; st < S; ++st) {
        k = per_step(k0);
        ws = ws0 + (k - k0);
        double* u = p.u + k;
        for (int c = 0; c < (H - 1) * I; ++c) u[(int64_t)c * ld] = u[(int64_t)(c + I) * ld];   // mpc.h:231-232
        f = polish::polish_instance<I>(p, H, k, ws, wn);
        if (f) break;
        r.step = st;
        k = per_step(k0);
        rollout_step_tail<double, Plant>(r, k);
        if (r.iters_out) r.iters_out[(int64_t)st * lo + k] = 0;
        if (p.status) p.status += lo;
        if (p.res_in) p.res_in += lo;
        if (p.res_out) p.res_out += lo;
    }
    *first = st;
    if (st == S) return 0u;
    k = per_step(k0);
    double* u = p.u + k;
    for (int c = 0; c < H * I; ++c) u[(int64_t)c * ld] = 0.0;
    for (int t = st; t < S; ++t) {
        const int64_t row = (int64_t)t * lo + k;   // row of a one-component output; others scale t
        for (int j = 0; j < I; ++j) ((double*)r.controls_out)[((int64_t)t * I + j) * lo + k] = 0.0;
        if (r.states_out)
            for (int j = 0; j < 2; ++j) ((double*)r.states_out)[((int64_t)t * 2 + j) * lo + k] = 0.0;
        if (r.sequences_out)
            for (int c = 0; c < H * I; ++c) ((double*)r.sequences_out)[((int64_t)t * H * I + c) * lo + k] = 0.0;
        if (r.iters_out) r.iters_out[row] = 0;
        if (a.p.status) a.p.status[row] = -1;
        if (a.p.res_in) a.p.res_in[row] = 0.0;
        if (a.p.res_out) a.p.res_out[row] = 0.0;
    }
    return f;
}

// What a lane does with its instance's result: first_unverified, the flags, and its place in the fallback's queue
// (mpc_newton_fallback.h).  Shared by the two kernels below.
__device__ __forceinline__ void newton_finish(const NewtonArgs& a, int64_t k, uint32_t f, int32_t first, uint32_t* flags) {
    a.first_unverified[k] = first;
    const uint32_t raise = raised_flags(a.raise_not_polished, f);
    if (raise) atomicOr(flags, raise);
    fallback_enqueue(a.fb_index, a.fb_count, k, f);
}

template <int I>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(I == 2 ? 4 : 5))) void rollout_newton_kernel(NewtonArgs a, double* ws, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.p.n) return;
    int32_t first;
    const uint32_t f = newton_instance<I>(a, k, ws + k, a.p.n, &first);
    newton_finish(a, k, f, first, flags);
}

// ... against a separate plant (tpc_mpc_rollout_plant): the same lane, the same occupancy
template <int I>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(I == 2 ? 4 : 5))) void rollout_plant_newton_kernel(NewtonArgs a, double* ws, uint32_t* flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.p.n) return;
    int32_t first;
    const uint32_t f = newton_instance<I, true>(a, k, ws + k, a.p.n, &first);
    newton_finish(a, k, f, first, flags);
}

// column index[j] of the batch <-> column j of the compact batch, every row of every set
template <bool kScatter>
__global__ __launch_bounds__(256) void rollout_newton_move_kernel(NewtonMove m) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m.count) return;
    const int64_t k = m.index[j];
    for (int q = 0; q < m.sets; ++q) {
        const NewtonRows& s = m.set[q];
        const int64_t from = kScatter ? j : k, to = kScatter ? k : j;
        if (s.bytes == 8) {
            const double* src = (const double*)s.src + from;
            double* dst = (double*)s.dst + to;
            for (int64_t r = 0; r < s.rows; ++r) dst[r * s.ld_dst] = src[r * s.ld_src];
        } else {
            const int32_t* src = (const int32_t*)s.src + from;
            int32_t* dst = (int32_t*)s.dst + to;
            for (int64_t r = 0; r < s.rows; ++r) dst[r * s.ld_dst] = src[r * s.ld_src];
        }
    }
}

__global__ void rollout_newton_flags_kernel(uint32_t* dst, const uint32_t* src) {
    const uint32_t f = *src;
    if (f) atomicOr(dst, f);
}

}  // namespace

int rollout_grad_block(int64_t n);   // mpc_rollout_grad.hip: the largest of 256, 128, 64 that gives a block per CU

// ws holds polish_scratch_bytes(I, H, n).  A lane's time is its own chain of steps and rounds: polish_general's block.
hipError_t rollout_newton(int I, const NewtonArgs& a, void* ws, uint32_t* flags, hipStream_t s) {
    if (a.p.n <= 0) return hipSuccess;
    const int block = rollout_grad_block(a.p.n);
    const unsigned grid = (unsigned)((a.p.n + block - 1) / block);
    if (a.plant && I == 2)
        hipLaunchKernelGGL(rollout_plant_newton_kernel<2>, dim3(grid), dim3(block), 0, s, a, (double*)ws, flags);
    else if (a.plant)
        hipLaunchKernelGGL(rollout_plant_newton_kernel<1>, dim3(grid), dim3(block), 0, s, a, (double*)ws, flags);
    else if (I == 2)
        hipLaunchKernelGGL(rollout_newton_kernel<2>, dim3(grid), dim3(block), 0, s, a, (double*)ws, flags);
    else
        hipLaunchKernelGGL(rollout_newton_kernel<1>, dim3(grid), dim3(block), 0, s, a, (double*)ws, flags);
    return hipGetLastError();
}

// HOST arrays, on the calling thread: the same newton_instance() per instance; returns the OR of the flags
uint32_t rollout_newton_host(int I, const NewtonArgs& a) {
    std::vector<double> ws((size_t)polish::slots(I) * a.r.H);
    uint32_t flags = 0;
    for (int64_t k = 0; k < a.p.n; ++k) {
        int32_t first;
        uint32_t f;
        if (a.plant)
            f = I == 2 ? newton_instance<2, true>(a, k, ws.data(), 1, &first)
                       : newton_instance<1, true>(a, k, ws.data(), 1, &first);
        else
            f = I == 2 ? newton_instance<2>(a, k, ws.data(), 1, &first) : newton_instance<1>(a, k, ws.data(), 1, &first);
        a.first_unverified[k] = first;
        flags |= raised_flags(a.raise_not_polished, f);
    }
    return flags;
}

hipError_t rollout_newton_move(const NewtonMove& m, bool scatter, hipStream_t s) {
    if (m.count <= 0) return hipSuccess;
    const int block = 256;
    const unsigned grid = (unsigned)((m.count + block - 1) / block);
    if (scatter) hipLaunchKernelGGL(rollout_newton_move_kernel<true>, dim3(grid), dim3(block), 0, s, m);
    else hipLaunchKernelGGL(rollout_newton_move_kernel<false>, dim3(grid), dim3(block), 0, s, m);
    return hipGetLastError();
}

hipError_t rollout_newton_merge_flags(uint32_t* dst, const uint32_t* src, hipStream_t s) {
    hipLaunchKernelGGL(rollout_newton_flags_kernel, dim3(1), dim3(1), 0, s, dst, src);
    return hipGetLastError();
}

}  // namespace tpc
