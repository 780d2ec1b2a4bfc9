// Polish of the general form (tpc_mpc_polish_batch_general, include/tpc_mpc.h): the arithmetic of ONE instance, shared
// by the gfx950 kernel (mpc_polish.hip) and the host path of the same entry.  As in mpc_grad_model.h every fused
// operation is an explicit fma() and the translation units are built with -ffp-contract=off, so the kernel and the host
// path give the same bits (tests/test_polish_gpu.py holds them to it).
//
// Given a control sequence u, a few safeguarded Newton rounds on dlib's box QP (mpc.h:255-283, df = H u + MM):
//   u <- clamp(u, lower, upper)
//   for round = 0 .. max_rounds:
//       df from u;  (t, j) is BLOCKED iff (u <= lower_j && df > 0) || (u >= upper_j && df < 0) || lower_j == upper_j
//       (dlib's mask, mpc.h:298-299), F the rest;  res = max |df| over F (0 when F is empty)
//       if res <= tol: status = round, return u                     -- a verified KKT point of the box QP
//       if round == max_rounds: break
//       safeguard: if the previous round was a regular one and did not lower res, this round is an INNER round:
//                  F loses the components that sit on a bound (they stay there); the next round is regular again
//       w = H_FF^-1 df_F (w = 0 off F), u <- clamp(u - w, lower, upper)
//   status = -1, the caller's sequence is left as it was
// The acceptance test is the proof: H is positive definite (R > 0), so a u with res <= tol under dlib's mask satisfies
// the KKT conditions of the convex QP to tol whatever path led there.
//
// Per round three passes over the horizon and the two of grad::riccati_passes, no per-step array in registers or
// private memory.  The workspace has slots(I) doubles per step, laid out as in mpc_grad_model.h:
//   gradient pass, forward:   x_{t+1} -> slots 0, 1
//   gradient pass, backward:  p_t = A' p_{t+1} + Q (x_{t+1} - target_t), df_t = B' p_t + R u_t -> slot 2 I + j
//   riccati_passes:           g = df read from slot 2 I + j (before the step's feed-forward is written there),
//                             leaves w in slot 4 + j
//   update:                   u in slot 4 + I + j, the working copy -- the caller's array is written on success only
// The rounds are newton_rounds() below, the one copy: polish_instance() calls it with the targets read from the caller's
// array, the exact compact solve (mpc_newton_compact_model.h, exact_instance) with its two target values in registers.
// tests/golden/newton_rounds_parent.npz pins the bits of both callers to the code before they shared it.
#pragma once

#include "mpc_grad_model.h"

namespace tpc {
namespace polish {

using grad::gabs;
using grad::gfinite;
using grad::gfma;

// SoA arrays, fp64, component c of instance k at base[c * ld + k]; u is read and, on success, written
struct Args {
    int64_t n, ld;
    const double *A, *B, *C, *Q, *R, *lo, *hi, *x0, *targets;
    double *u, *u0;
    double tol;
    int32_t max_rounds;
    int32_t* status;
    double *res_in, *res_out;
};

// workspace doubles per step: the gradient workspace plus the working copy of u
TPC_GRAD_HD constexpr int slots(int I) { return grad::slots(I) + I; }

TPC_GRAD_HD double clampd(double u, double lo, double hi) { return u < lo ? lo : (u > hi ? hi : u); }

// For the closed loops that run every step of an instance in one lane (mpc_rollout_newton.hip, mpc_compact_loop_model.h):
// the step loop must cost no registers beyond one step's.  Without this the compiler hoists every array's per-lane
// address (base + k, two VGPRs each, some forty of them in the general form) out of the loop and the kernel loses half
// its occupancy.  An instance index the optimiser cannot see through is re-made per step, so the addresses are formed
// where used.
TPC_GRAD_HD int64_t per_step(int64_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(k));
#endif
    return k;
}

// The rounds, on the working copy the caller has put in slots 4 + I + j.  tg_at(t, c) is component c of step t's target.
// Returns the round at which res <= tol, with that res in res_out and the verified sequence in the working copy; -1 when
// a df overflowed or max_rounds were used up (res_out is left alone).  res_in is round 0's residual either way.
// H may be a compile-time constant of the caller's (mpc_newton_compact.hip): the function is inlined, every loop over
// the horizon below then unrolls, and a ws that is an array of the lane's own stays in registers.
template <int I, class TG>
TPC_GRAD_HD int32_t newton_rounds(const grad::Model& m, int H, double xs0, double xs1, TG tg_at, double tol,
                                  int32_t max_rounds, double* ws, int64_t wn, double& res_in, double& res_out) {
    auto slot = [&](int q, int t) -> double& { return ws[((int64_t)q * H + t) * wn]; };
    constexpr int kU = 4 + I, kDf = 2 * I;   // first slot of the working copy / of df
    auto blocked = [&](int j, double u, double df) {   // dlib's mask, mpc.h:298-299
        return (u <= m.lo[j] && df > 0.0) || (u >= m.hi[j] && df < 0.0) || m.lo[j] == m.hi[j];
    };
    double prev = 0.0;
    bool inner = false;
    res_in = 0.0;
    for (int32_t round = 0;; ++round) {
        // ---- gradient, forward: x_{t+1}
        double x0 = xs0, x1 = xs1;
        for (int t = 0; t < H; ++t) {
            double y0 = gfma(m.a00, x0, gfma(m.a01, x1, m.c0)), y1 = gfma(m.a10, x0, gfma(m.a11, x1, m.c1));
#pragma unroll
            for (int j = 0; j < I; ++j) {
                const double u = slot(kU + j, t);
                y0 = gfma(m.b0[j], u, y0);
                y1 = gfma(m.b1[j], u, y1);
            }
            x0 = y0; x1 = y1;
            slot(0, t) = x0; slot(1, t) = x1;
        }
        // ---- gradient, backward: costate, df, the mask, the residual
        double P0 = 0.0, P1 = 0.0, res = 0.0;
        bool okdf = true;
        for (int t = H - 1; t >= 0; --t) {
            const double e0 = slot(0, t) - tg_at(t, 0), e1 = slot(1, t) - tg_at(t, 1);
            const double p0 = gfma(m.a00, P0, gfma(m.a10, P1, m.q0 * e0)), p1 = gfma(m.a01, P0, gfma(m.a11, P1, m.q1 * e1));
            P0 = p0; P1 = p1;
#pragma unroll
            for (int j = 0; j < I; ++j) {
                const double u = slot(kU + j, t);
                const double df = gfma(m.b0[j], p0, gfma(m.b1[j], p1, m.r[j] * u));
                slot(kDf + j, t) = df;
                okdf = okdf && gfinite(df);
                if (!blocked(j, u, df)) res = gabs(df) > res ? gabs(df) : res;
            }
        }
        if (round == 0) res_in = res;
        if (!okdf) return -1;   // an intermediate overflowed
        if (res <= tol) {
            res_out = res;
            return round;
        }
        if (round >= max_rounds) return -1;
        inner = !inner && round > 0 && !(res < prev);
        prev = res;

        // ---- w = H_FF^-1 df_F, then the clamped step
        bool f2 = true;
        double y0, y1, d0, d1;
        grad::riccati_passes<I>(
            m, H, xs0, xs1, [&](int t, int j) { return slot(kU + j, t); }, [&](int t, int j) { return slot(kDf + j, t); },
            [&](int j, double u, double df) { return !blocked(j, u, df) && !(inner && (u <= m.lo[j] || u >= m.hi[j])); },
            ws, wn, f2, y0, y1, d0, d1);
        for (int t = 0; t < H; ++t)
#pragma unroll
            for (int j = 0; j < I; ++j) slot(kU + j, t) = clampd(slot(kU + j, t) - slot(4 + j, t), m.lo[j], m.hi[j]);
    }
}

// One instance.  ws points at the instance's first workspace element (ws[(q * H + t) * wn]).  Returns its
// TPC_MPC_FLAG_* bits: 0x1 non-finite, 0x4 bad model (both: nothing run, status -1), 0x8 not polished.
template <int I>
TPC_GRAD_HD uint32_t polish_instance(const Args& a, int H, int64_t k, double* ws, int64_t wn) {
    const int64_t ld = a.ld;
    auto in = [&](const double* base, int c) -> double { return base[(int64_t)c * ld + k]; };
    auto slot = [&](int q, int t) -> double& { return ws[((int64_t)q * H + t) * wn]; };
    const grad::Model m = grad::load_model<I>(a.A, a.B, a.C, a.Q, a.R, a.lo, a.hi, ld, k);
    const double xs0 = in(a.x0, 0), xs1 = in(a.x0, 1);
    bool fin = m.fin && gfinite(xs0) && gfinite(xs1);
    constexpr int kU = 4 + I;   // first slot of the working copy

    for (int t = 0; t < H; ++t) {
        fin = fin && gfinite(in(a.targets, 2 * t)) && gfinite(in(a.targets, 2 * t + 1));
#pragma unroll
        for (int j = 0; j < I; ++j) {
            const double u = in(a.u, t * I + j);
            fin = fin && gfinite(u);
            slot(kU + j, t) = clampd(u, m.lo[j], m.hi[j]);
        }
    }
    auto finish = [&](int32_t status, double r_in, double r_out) {
        if (a.status) a.status[k] = status;
        if (a.res_in) a.res_in[k] = r_in;
        if (a.res_out) a.res_out[k] = r_out;
        if (a.u0)
#pragma unroll
            for (int j = 0; j < I; ++j) a.u0[(int64_t)j * ld + k] = status >= 0 ? slot(kU + j, 0) : in(a.u, j);
    };
    const uint32_t bad = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    if (bad) {
        finish(-1, 0.0, 0.0);
        return bad;
    }

    double res_in = 0.0, res_out = 0.0;
    const int32_t round =
        newton_rounds<I>(m, H, xs0, xs1, [&](int t, int c) { return in(a.targets, 2 * t + c); }, a.tol, a.max_rounds, ws,
                         wn, res_in, res_out);
    if (round >= 0) {
        for (int t = 0; t < H; ++t)
#pragma unroll
            for (int j = 0; j < I; ++j) a.u[(int64_t)(t * I + j) * ld + k] = slot(kU + j, t);
        finish(round, res_in, res_out);
        return 0u;
    }
    // the caller's sequence stands, so its residual does: residual_out = residual_in.  (The exact compact solve, whose
    // unverified outputs are zeros, reports 0.0 here -- the one difference between the two callers' outputs.)
    finish(-1, res_in, res_in);
    return 0x8u;
}

}  // namespace polish
}  // namespace tpc
