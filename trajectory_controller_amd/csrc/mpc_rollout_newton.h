// The Newton-first closed loop (tpc_mpc_rollout_newton, include/tpc_mpc.h): what tpc_mpc_api.cpp hands to the kernels
// and the host path of mpc_rollout_newton.hip.
#pragma once

#include "mpc_internal.h"
#include "mpc_polish_model.h"

namespace tpc {

// Phase 1.  p and r describe the same working set (p.u = r.controls, p.x0 = r.x, p.targets = r.targets, p.ld = r.ld),
// which the loop updates in place; p.status / res_in / res_out point at step 0's row of the per-step outputs (ld_out
// apart, like iters_out) or are null.  r.iters_step is null: the loop writes iters_out itself.
struct NewtonArgs {
    polish::Args p;
    RolloutStepArgs r;
    int32_t* first_unverified;   // [n]
    int32_t* fb_index;           // [n] the instances for the fallback, in no particular order; null: not collected
    uint32_t* fb_count;          // how many
    int32_t raise_not_polished;  // FALLBACK_NONE: an unverified instance raises TPC_MPC_FLAG_NOT_POLISHED here
    int32_t plant;               // tpc_mpc_rollout_plant: r.A, r.B, r.C are set by the caller (the plant's arrays) and
                                 // r.disturbance may be given; 0: the tail reads p's model, as tpc_mpc_rollout_newton
};

// Rows of `ld`-strided fp64 (or int32) SoA arrays moved between the batch (column index[j]) and the compact fallback
// batch (column j): gather reads the batch, scatter writes it.
struct NewtonRows {
    const void* src;
    void* dst;
    int64_t rows, ld_src, ld_dst;
    int32_t bytes;   // 8 or 4 per element
};
constexpr int kNewtonRowSets = 10;
struct NewtonMove {
    int64_t count;
    const int32_t* index;
    int sets;
    NewtonRows set[kNewtonRowSets];
};

hipError_t rollout_newton(int I, const NewtonArgs& a, void* ws, uint32_t* flags, hipStream_t s);
uint32_t rollout_newton_host(int I, const NewtonArgs& a);
hipError_t rollout_newton_move(const NewtonMove& m, bool scatter, hipStream_t s);
hipError_t rollout_newton_merge_flags(uint32_t* dst, const uint32_t* src, hipStream_t s);

}  // namespace tpc
