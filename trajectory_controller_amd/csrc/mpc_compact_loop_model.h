// The compact closed loop (tpc_mpc_rollout_compact_exact, include/tpc_mpc.h): phase 1 of ONE instance, every step,
// shared by the gfx950 kernels (mpc_compact_loop.hip) and the host path of the same entry.  It is the Newton-first
// closed loop (mpc_rollout_newton.hip, newton_instance) on the reference controller's model:
//   - the model is built once, from v and the call's parameters, in registers (cexact::build_model); the state is two
//     doubles, the target two doubles -- every one of the H targets is (dy, dphi) at every step, which is what the
//     general loop's target shift leaves when no new last target is given;
//   - the carried controls are the working copy of the rounds (slots kU + j): dlib's shift (mpc.h:231-232) moves them
//     there, t <- t + 1 with the last step kept, and the clamp of the polish follows;
//   - the rounds are polish::newton_rounds<2>, the one copy;
//   - a verified step moves the state in rollout_step_tail's arithmetic on the expanded values, literally -- the
//     multiplies by 1.0 and 0.0 and the "+ 0.0" are kept, because they decide signed zeros and what an Inf becomes.
// Nothing is read from memory inside the step loop but the workspace slots, and the only stores are the outputs.
// An instance carried to the end equals tpc_mpc_rollout_newton on the expanded arrays bit for bit
// (tests/test_compact_loop_host.py).  Explicit fma() only; the unit is built with -ffp-contract=off.
#pragma once

#include "mpc_newton_compact_model.h"

namespace tpc {
namespace cloop {

using cexact::kI;
using grad::gfinite;
using polish::clampd;
using polish::per_step;   // the step loop costs no registers beyond one step's

// c: the single solve's arguments, of which the loop reads n, v, dy, dphi, the ten model values, tol, max_rounds,
// raise_not_polished and the fallback's queue (its output pointers are unused).  The per-step outputs are rows ld_out
// apart: controls [S*2] (required), states [S*2], sequences [S*H*2], status / res_in / res_out [S], first [n], each
// of which may be null.
struct Args {
    cexact::Args c;
    const double* x0;   // [2] rows ld_x0 apart; null: zeros
    int64_t ld_x0;
    int32_t steps;
    double *controls, *states, *sequences;
    int32_t* status;
    double *res_in, *res_out;
    int32_t* first;
    int64_t ld_out;
};

// One instance, every step.  HC > 0: the horizon, at compile time (Hrt is ignored; ws0 is then an array of the lane's
// own, wn == 1, whose every index is a constant); HC == 0: Hrt.  Returns the flags of the step it stopped at (0:
// verified at every step; 0x1 non-finite, 0x4 bad model, 0x8 not verified) and that step in *first.  Rows of the
// per-step outputs from *first on are cleared: status -1, everything else 0.
template <int HC>
TPC_GRAD_HD uint32_t loop_instance(const Args& a, int Hrt, int64_t k0, double* ws0, int64_t wn, int32_t* first) {
    constexpr int I = kI;
    constexpr int kU = 4 + I;   // first slot of the working copy
    const int H = HC > 0 ? HC : Hrt, S = a.steps;
    const int64_t lo = a.ld_out;
    double* ws = ws0;
    auto slot = [&](int q, int t) -> double& { return ws[((int64_t)q * H + t) * wn]; };
    const double tg0 = a.c.dy[k0], tg1 = a.c.dphi[k0];
    const grad::Model m = cexact::build_model(a.c, a.c.v[k0]);
    double xs0 = a.x0 ? a.x0[k0] : 0.0, xs1 = a.x0 ? a.x0[a.ld_x0 + k0] : 0.0;
    const bool fin0 = m.fin && gfinite(tg0) && gfinite(tg1);

    for (int t = 0; t < H; ++t)   // no carried controls
#pragma unroll
        for (int j = 0; j < I; ++j) slot(kU + j, t) = 0.0;

    uint32_t f = 0;
    int st = 0;
    for (; st < S; ++st) {
        const int64_t k = per_step(k0);
        if (HC == 0) ws = ws0 + (k - k0);
        for (int t = 0; t + 1 < H; ++t)   // mpc.h:231-232
#pragma unroll
            for (int j = 0; j < I; ++j) slot(kU + j, t) = slot(kU + j, t + 1);
        // the polish's start: the clamp.  (Its finiteness test of the sequence is met by construction: zeros, or a
        // verified sequence, whose df = .. + r u is finite with r > 0.)
        for (int t = 0; t < H; ++t)
#pragma unroll
            for (int j = 0; j < I; ++j) slot(kU + j, t) = clampd(slot(kU + j, t), m.lo[j], m.hi[j]);
        const bool fin = fin0 && gfinite(xs0) && gfinite(xs1);
        f = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
        if (f) break;
        double res_in = 0.0, res_out = 0.0;
        const int32_t round = polish::newton_rounds<I>(
            m, H, xs0, xs1, [&](int, int c) { return c == 0 ? tg0 : tg1; }, a.c.tol, a.c.max_rounds, ws, wn, res_in,
            res_out);
        if (round < 0) {
            f = 0x8u;
            break;
        }
        // rollout_step_tail on the expanded values: x <- A x + B u0 + C  (test/mpc.cpp:314), no fused operation
        const double u0 = slot(kU, 0), u1 = slot(kU + 1, 0);
        double bu0 = m.b0[0] * u0, bu1 = m.b1[0] * u0;
        bu0 = bu0 + m.b0[1] * u1;
        bu1 = bu1 + m.b1[1] * u1;
        const double n0 = ((m.a00 * xs0 + m.a01 * xs1) + bu0) + m.c0;
        const double n1 = ((m.a10 * xs0 + m.a11 * xs1) + bu1) + m.c1;
        xs0 = n0; xs1 = n1;
        const int64_t row = (int64_t)st * lo + k;   // row of a one-component output; the others scale st
        a.controls[((int64_t)st * I) * lo + k] = u0;
        a.controls[((int64_t)st * I + 1) * lo + k] = u1;
        if (a.states) {
            a.states[((int64_t)st * 2) * lo + k] = n0;
            a.states[((int64_t)st * 2 + 1) * lo + k] = n1;
        }
        if (a.sequences) {
            double* q = a.sequences + (int64_t)st * H * I * lo + k;
            for (int t = 0; t < H; ++t)
#pragma unroll
                for (int j = 0; j < I; ++j) q[(int64_t)(t * I + j) * lo] = slot(kU + j, t);
        }
        if (a.status) a.status[row] = round;
        if (a.res_in) a.res_in[row] = res_in;
        if (a.res_out) a.res_out[row] = res_out;
    }
    *first = st;
    if (st == S) return 0u;
    const int64_t k = per_step(k0);
    for (int t = st; t < S; ++t) {
        const int64_t row = (int64_t)t * lo + k;
#pragma unroll
        for (int j = 0; j < I; ++j) a.controls[((int64_t)t * I + j) * lo + k] = 0.0;
        if (a.states)
#pragma unroll
            for (int j = 0; j < 2; ++j) a.states[((int64_t)t * 2 + j) * lo + k] = 0.0;
        if (a.sequences)
            for (int c = 0; c < H * I; ++c) a.sequences[((int64_t)t * H * I + c) * lo + k] = 0.0;
        if (a.status) a.status[row] = -1;
        if (a.res_in) a.res_in[row] = 0.0;
        if (a.res_out) a.res_out[row] = 0.0;
    }
    return f;
}

}  // namespace cloop
}  // namespace tpc
