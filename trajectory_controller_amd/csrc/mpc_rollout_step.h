// The step tail of the closed loops (tpc_mpc_rollout, tpc_mpc_rollout_record, tpc_mpc_rollout_polished): what the
// caller of dlib::mpc does between two operator() calls (reference: dlib_files/dlib/test/mpc.cpp:301-316) plus the
// target shift operator() performs itself (mpc.h:236-237), for instance k.  Shared by rollout_step_kernel
// (mpc_rollout.hip), the fused polish + step kernel (mpc_rollout_polish.hip) and the Newton-first loop
// (mpc_rollout_newton.hip, kernel and host path); no fused multiply-add in it, and the units that include it are built
// with -ffp-contract=off, so all give the same bits.
// With Plant (tpc_mpc_rollout_plant) a.A, a.B, a.C are the plant's arrays and row `step` of a.disturbance, when there
// is one, is added to the new state: one more plain add after the parent's arithmetic, none without a disturbance.
#pragma once

#include "mpc_internal.h"

namespace tpc {

template <typename T, bool Plant = false>
__host__ __device__ __forceinline__ void rollout_step_tail(const RolloutStepArgs& a, int64_t k) {
    const int64_t ld = a.ld;
    const T* A = (const T*)a.A + k;
    const T* B = (const T*)a.B + k;
    const T* Cc = (const T*)a.C + k;
    T* x = (T*)a.x + k;
    const T* u = (const T*)a.controls + k;   // controls[0](j) at component j
    // record u0 and advance the plant: x <- A*x + B*u + C  (test/mpc.cpp:314)
    T bu0 = B[0] * u[0], bu1 = B[(int64_t)a.I * ld] * u[0];
    if (a.I == 2) { bu0 = bu0 + B[ld] * u[ld]; bu1 = bu1 + B[3 * ld] * u[ld]; }
    const T x0 = x[0], x1 = x[ld];
    T n0 = ((A[0] * x0 + A[ld] * x1) + bu0) + Cc[0];
    T n1 = ((A[2 * ld] * x0 + A[3 * ld] * x1) + bu1) + Cc[ld];
    if (Plant && a.disturbance) {
        const T* d = (const T*)a.disturbance + k;
        n0 = n0 + d[(2 * (int64_t)a.step) * a.ld_d];
        n1 = n1 + d[(2 * (int64_t)a.step + 1) * a.ld_d];
    }
    x[0] = n0; x[ld] = n1;
    const int64_t lo = a.ld_out;
    for (int j = 0; j < a.I; ++j) ((T*)a.controls_out)[((int64_t)a.step * a.I + j) * lo + k] = u[(int64_t)j * ld];
    if (a.states_out) {
        ((T*)a.states_out)[((int64_t)a.step * 2) * lo + k] = n0;
        ((T*)a.states_out)[((int64_t)a.step * 2 + 1) * lo + k] = n1;
    }
    if (a.iters_out && a.iters_step) a.iters_out[(int64_t)a.step * lo + k] = a.iters_step[k];
    if (a.sequences_out) {   // the whole sequence U_step, before the next solve shifts it
        const int64_t hi = (int64_t)a.H * a.I;
        T* q = (T*)a.sequences_out + (int64_t)a.step * hi * lo + k;
        for (int64_t c = 0; c < hi; ++c) q[c * lo] = u[c * ld];
    }
    // operator()'s target shift (mpc.h:236-237), then the caller's set_last_target for the next call
    T* t = (T*)a.targets + k;
    for (int i = 1; i < a.H; ++i) {
        t[(int64_t)(2 * (i - 1)) * ld] = t[(int64_t)(2 * i) * ld];
        t[(int64_t)(2 * (i - 1) + 1) * ld] = t[(int64_t)(2 * i + 1) * ld];
    }
    if (a.new_last_targets && a.step + 1 < a.steps) {
        const T* nl = (const T*)a.new_last_targets + k;
        t[(int64_t)(2 * (a.H - 1)) * ld] = nl[(2 * ((int64_t)a.step + 1)) * a.ld_nlt];
        t[(int64_t)(2 * (a.H - 1) + 1) * ld] = nl[(2 * ((int64_t)a.step + 1) + 1) * a.ld_nlt];
    }
}

}  // namespace tpc
