// The device pieces that the Newton-first entries share for their fallback (tpc_mpc_api.cpp, newton_two_phase, says
// how the two phases fit together): which flags a lane raises, the wave-aggregated queue of the instances phase 1 could
// not verify, and the expansion of a compact instance to the general form's rows.  Used by mpc_rollout_newton.hip,
// mpc_newton_compact.hip and mpc_compact_loop.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpc_grad_model.h"

namespace tpc {

// What an instance with the flags f raises: with the fallback (raise_not_polished false) "not polished" (0x8) is the
// fallback's to settle, not the call's to report
__host__ __device__ inline uint32_t raised_flags(bool raise_not_polished, uint32_t f) {
    return raise_not_polished ? f : (f & ~0x8u);
}

// The compact batch of the compact entries' fallback: instance index[j] of the call <-> column j, leading dimension ld,
// the general form's nine model rows (I = 2).
struct FallbackBatch {
    int64_t count, ld;
    const int32_t* index;
    int H;
    double *A, *B, *C, *Q, *R, *lo, *hi, *x0, *targets;
};

#if defined(__HIPCC__)
// The fallback's queue: instance k joins it when it is not verified and nothing else is wrong with it (f == 0x8).  One
// atomicAdd per wavefront; every lane that reaches the end of a phase-1 kernel calls it.  fb_index null: no queue.
__device__ __forceinline__ void fallback_enqueue(int32_t* fb_index, uint32_t* fb_count, int64_t k, uint32_t f) {
    if (!fb_index) return;
    const bool fb = f == 0x8u;
    const unsigned long long m = __ballot(fb);
    if (!m) return;
    const int lane = __lane_id(), leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(fb_count, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    if (fb) fb_index[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)k;
}

// Column j of the compact batch: the model m, H copies of the target (tg0, tg1) and the state (x00, x01)
__device__ inline void expand_general(const grad::Model& m, double tg0, double tg1, double x00, double x01,
                                      const FallbackBatch& b, int64_t j) {
    const int64_t ld = b.ld;
    auto out = [&](double* base, int c, double x) { base[(int64_t)c * ld + j] = x; };
    out(b.A, 0, m.a00); out(b.A, 1, m.a01); out(b.A, 2, m.a10); out(b.A, 3, m.a11);
    out(b.B, 0, m.b0[0]); out(b.B, 1, m.b0[1]); out(b.B, 2, m.b1[0]); out(b.B, 3, m.b1[1]);
    out(b.C, 0, m.c0); out(b.C, 1, m.c1);
    out(b.Q, 0, m.q0); out(b.Q, 1, m.q1);
    out(b.x0, 0, x00); out(b.x0, 1, x01);
    for (int c = 0; c < 2; ++c) { out(b.R, c, m.r[c]); out(b.lo, c, m.lo[c]); out(b.hi, c, m.hi[c]); }
    for (int t = 0; t < b.H; ++t) { out(b.targets, 2 * t, tg0); out(b.targets, 2 * t + 1, tg1); }
}
#endif

}  // namespace tpc
