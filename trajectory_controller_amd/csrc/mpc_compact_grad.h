// Backward pass of the exact compact solve (tpc_mpc_solve_batch_compact_exact_backward, include/tpc_mpc.h): what
// tpc_mpc_api.cpp hands to the kernels and the host path of mpc_compact_grad.hip.
#pragma once

#include "mpc_internal.h"
#include "mpc_compact_grad_model.h"

namespace tpc {

// true: a kernel with the horizon at compile time and the per-step values in registers serves H
bool compact_grad_in_registers(int H);
// the launch's blocks: the partial rows of the shared-parameter sum, 10 doubles each
int64_t compact_grad_blocks(int64_t n);
// the per-step workspace of the launch (0 when compact_grad_in_registers(H))
int64_t compact_grad_scratch_bytes(int H, int64_t n);
// DEVICE arrays.  ws holds compact_grad_scratch_bytes(H, n); with dparams != null, partials holds
// 10 * compact_grad_blocks(n) doubles and dparams [10] receives their sum (one more launch)
hipError_t compact_grad(int H, const cgrad::Args& a, void* ws, double* partials, double* dparams, uint32_t* flags,
                        hipStream_t s);
// ... and on the calling thread, dparams (may be null) summed in ascending k; returns the OR of the flags
uint32_t compact_grad_host(int H, const cgrad::Args& a, double* dparams);

}  // namespace tpc
