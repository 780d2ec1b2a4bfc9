// The compact closed loop (tpc_mpc_rollout_compact_exact, include/tpc_mpc.h): what tpc_mpc_api.cpp hands to the
// kernels and the host path of mpc_compact_loop.hip.
#pragma once

#include "mpc_internal.h"
#include "mpc_compact_loop_model.h"
#include "mpc_newton_fallback.h"

namespace tpc {

// The fallback's compact batch.  Gather-expand writes the general form of the queued instances -- the model as
// cexact::build_model makes it, the call's x0 (zeros without one) and H copies of the target -- for the polished loop
// (rollout_impl), which starts from no carried controls itself; its per-step rows go back through rollout_newton_move.
using CompactLoopBatch = FallbackBatch;

// true: a kernel with the horizon at compile time and the whole loop in registers serves H
bool compact_loop_in_registers(int H);
// phase 1 on DEVICE arrays; ws holds polish_scratch_bytes(2, H, n) (not touched when compact_loop_in_registers(H))
hipError_t compact_loop(int H, const cloop::Args& a, void* ws, uint32_t* flags, hipStream_t s);
// ... and on the calling thread; returns the OR of the flags
uint32_t compact_loop_host(int H, const cloop::Args& a);
hipError_t compact_loop_gather(const cloop::Args& a, const CompactLoopBatch& b, hipStream_t s);

}  // namespace tpc
