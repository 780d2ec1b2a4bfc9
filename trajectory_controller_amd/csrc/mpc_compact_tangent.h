// Forward-mode derivative of the exact compact solve (tpc_mpc_solve_batch_compact_exact_forward, include/tpc_mpc.h): what
// tpc_mpc_api.cpp hands to the kernels and the host path of mpc_compact_tangent.hip.
#pragma once

#include "mpc_internal.h"
#include "mpc_compact_tangent_model.h"

namespace tpc {

// true: a kernel with the horizon at compile time and the per-step values in registers serves H (row 0 only)
bool compact_tangent_in_registers(int H, bool whole);
// the per-step workspace of the launch (0 when compact_tangent_in_registers(H, whole))
int64_t compact_tangent_scratch_bytes(int H, int64_t n, int K, bool whole);
// DEVICE arrays, one lane per (direction, instance); a.tseq != null: the whole tangent sequence.  ws holds
// compact_tangent_scratch_bytes(H, n, K, a.tseq != null)
hipError_t compact_tangent(int H, const ctan::Args& a, void* ws, uint32_t* flags, hipStream_t s);
// ... and on the calling thread; returns the OR of the flags
uint32_t compact_tangent_host(int H, const ctan::Args& a);

}  // namespace tpc
