// The compact closed loop (tpc_mpc_rollout_compact_exact, include/tpc_mpc.h): what tpc_mpc_api.cpp hands to the
// kernels and the host path of mpc_compact_loop.hip.
#pragma once

#include "mpc_internal.h"
#include "mpc_compact_loop_model.h"

namespace tpc {

// The fallback's compact batch: instance index[j] of the call <-> column j, leading dimension ld.  Gather-expand
// writes the general form of those instances -- the model as cexact::build_model makes it, the call's x0 (zeros without
// one) and H copies of the target -- for the polished loop (rollout_impl), which starts from no carried controls
// itself; its per-step rows go back through rollout_newton_move.
struct CompactLoopBatch {
    int64_t count, ld;
    const int32_t* index;
    int H;
    double *A, *B, *C, *Q, *R, *lo, *hi, *x0, *targets;
};

// true: a kernel with the horizon at compile time and the whole loop in registers serves H
bool compact_loop_in_registers(int H);
// phase 1 on DEVICE arrays; ws holds polish_scratch_bytes(2, H, n) (not touched when compact_loop_in_registers(H))
hipError_t compact_loop(int H, const cloop::Args& a, void* ws, uint32_t* flags, hipStream_t s);
// ... and on the calling thread; returns the OR of the flags
uint32_t compact_loop_host(int H, const cloop::Args& a);
hipError_t compact_loop_gather(const cloop::Args& a, const CompactLoopBatch& b, hipStream_t s);

}  // namespace tpc
