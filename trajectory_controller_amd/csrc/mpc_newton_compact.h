// The exact compact solve (tpc_mpc_solve_batch_compact_exact, include/tpc_mpc.h): what tpc_mpc_api.cpp hands to the
// kernels and the host path of mpc_newton_compact.hip.
#pragma once

#include "mpc_internal.h"
#include "mpc_newton_compact_model.h"
#include "mpc_newton_fallback.h"

namespace tpc {

// The fallback's compact batch (FallbackBatch) and what the solve and the polish return for it.  Gather-expand writes
// the general form of the queued instances (the model as cexact::build_model makes it, x0 = 0, H copies of the
// target, zero controls); scatter reads what the solve and the polish left and writes the call's outputs (src's
// output pointers, null where the caller gave none) with fell_back = 1.
struct CompactExactBatch : FallbackBatch {
    double *controls, *u0, *res_in, *res_out;
    int32_t* status;
};

// true: a kernel with the horizon at compile time and the per-step values in registers serves H
bool compact_exact_in_registers(int H);
// phase 1 on DEVICE arrays; ws holds polish_scratch_bytes(2, H, n) (not touched when compact_exact_in_registers(H));
// a.start != null: the warm kernels (tpc_mpc_solve_batch_compact_exact_from), here and in compact_exact_host
hipError_t compact_exact(int H, const cexact::Args& a, void* ws, uint32_t* flags, hipStream_t s);
// ... and on the calling thread; returns the OR of the flags
uint32_t compact_exact_host(int H, const cexact::Args& a);
hipError_t compact_exact_gather(const cexact::Args& a, const CompactExactBatch& b, hipStream_t s);
hipError_t compact_exact_scatter(const cexact::Args& a, const CompactExactBatch& b, hipStream_t s);

}  // namespace tpc
