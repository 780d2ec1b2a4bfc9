// Backward pass of the compact closed loop (tpc_mpc_rollout_compact_exact_backward, include/tpc_mpc.h): what
// tpc_mpc_api.cpp hands to the kernels and the host path of mpc_compact_loop_grad.hip.
#pragma once

#include "mpc_internal.h"
#include "mpc_compact_loop_grad_model.h"

namespace tpc {

// true: a kernel with the horizon at compile time and the per-step values in registers serves H
bool cloop_grad_in_registers(int H);
// the launch's blocks: the partial rows of the shared-parameter sum, 10 doubles each
int64_t cloop_grad_blocks(int64_t n);
// the per-step workspace of the launch (0 when cloop_grad_in_registers(H)); one step's slots, reused by every step
int64_t cloop_grad_scratch_bytes(int H, int64_t n);
// DEVICE arrays.  ws holds cloop_grad_scratch_bytes(H, n); with dparams != null, partials holds
// 10 * cloop_grad_blocks(n) doubles and dparams [10] receives their sum (one more launch: compact_grad_reduce)
hipError_t cloop_grad(int H, const cloopgrad::Args& a, void* ws, double* partials, double* dparams, uint32_t* flags,
                      hipStream_t s);
// ... and on the calling thread, dparams (may be null) summed in ascending k; returns the OR of the flags
uint32_t cloop_grad_host(int H, const cloopgrad::Args& a, double* dparams);

}  // namespace tpc
