// Forward-mode derivatives of the general form (tpc_mpc_solve_batch_general_forward and tpc_mpc_rollout_forward,
// include/tpc_mpc.h): the arithmetic of ONE (direction, instance) pair, shared by the gfx950 kernels (mpc_tangent.hip,
// mpc_rollout_tangent.hip) and the host paths of the same entries.  As in mpc_grad_model.h every fused operation is an
// explicit fma() and the translation units are built with -ffp-contract=off, so the kernels and the host paths give
// the same bits (tests/test_rollout_tangent_gpu.py holds them to it).
//
// Model, costate p and active set as in mpc_grad_model.h.  A direction is a tangent of every input (tA .. tnlt, a
// null array is zero).  With u the recorded sequence of a solve from x_0, F its free components and
//   ub(t, j) = tlower_j / tupper_j on an active component (by the bound it sits on, lower first), 0 on F,
// the tangent of the solve is  tU = ub - w,  w = H_FF^-1 r_F (w = 0 off F), where r is the directional derivative of
// dlib's df = H u + MM along (the model's tangent, ub):
//   tx_{t+1} = tA x_t + A tx_t + tB u_t + B ub_t + tC                        (tx_0 given)
//   tp_t     = tA' p_{t+1} + A' tp_{t+1} + tQ e_{t+1} + Q (tx_{t+1} - tT_t)   (e_{t+1} = x_{t+1} - T_t)
//   r_t      = tB' p_t + B' tp_t + tR u_t + R ub_t
// and w comes from the masked Riccati sweep of mpc_grad_model.h (riccati_passes, pass 1, restated here operation for
// operation: sharing it would have meant touching a function whose bits three kernels are held to).
//
// Two passes over the horizon, no per-step array in registers or private memory: the per-step quantities live in a
// workspace of slots(I, whole) doubles per step, element (q, t) of a lane at ws[(q * H + t) * wn].
//   1. forward:  x_{t+1}, tx_{t+1} from u -> slots 0..3 of step t.
//   2. backward: p_t, tp_t, r_t and the Riccati step, fused.  The response dx of the Riccati problem starts at
//      dx_0 = 0, so w_0 = k_0, the feed-forward of step 0: row 0 of tU needs no stored gain and no third pass.
// Only the single solve returns the whole tU; it stores the gains and feed-forwards (slots 4 .. 4 + 3 I) and runs
//   3. forward:  w_t = K_t dx_t + k_t, dx_{t+1} = A dx_t + B w_t  (riccati_passes, pass 2)
// The closed loop needs row 0 only: rollout_instance() chains step() over the steps k = 0 .. S-1 with
//   tx_{k+1} = tA x_k + A tx_k + tB u0_k + B tu0_k + tC
// carried in registers, x_k read from the recorded states.
#pragma once

#include "mpc_grad_model.h"

namespace tpc {
namespace tangent {

using grad::gfinite;
using grad::gfma;
using grad::load_model;
using grad::Model;

// The K directions of a call: element (d, c, k) of a C-component array at base[(d * C + c) * ld + k]; null = zero
struct Dirs {
    const double *tA, *tB, *tC, *tQ, *tR, *tlo, *thi, *tx0, *ttargets, *tnlt;
};

// SoA arrays, fp64, of the single solve: the io's model, x0 and targets, the controls u [H*I], and tu [K*H*I]
struct Args {
    int64_t n, ld;
    int K;
    const double *A, *B, *C, *Q, *R, *lo, *hi, *x0, *targets, *u;
    Dirs t;
    double* tu;
};

// ... and of the closed loop: new_last_targets [steps*2] (may be null), the recorded sequences [steps*H*I] and states
// [steps*2], and the outputs tu [K*steps*I], tx [K*steps*2] (tx may be null)
struct RollArgs {
    int64_t n, ld;
    int steps, K;
    const double *A, *B, *C, *Q, *R, *lo, *hi, *x0, *targets, *nlt, *seq, *states;
    Dirs t;
    double *tu, *tx;
};

// The separate plant of tpc_mpc_rollout_plant_forward: tx_{k+1} = tAp x_k + Ap tx_k + tBp u0_k + Bp tu0_k + tCp + td_k.
// A, B, C are never null here and tA, tB, tC ([K*4], [K*2I], [K*2] stacked blocks, null = zero) are their tangents:
// the plant's, while the model's enter the step's QP only -- or, when the caller gave no plant, the controller's arrays
// and tangents again, which then move the state as in rollout_instance<I, false>.  The tangents are read through their
// arrays at the plant line (a choice between a read and a held value there costs the lane a wave of occupancy).
// td [K*steps*2] with the leading dimension ld_d, null = zero: no add at all.
struct RollPlant {
    const double *A, *B, *C, *tA, *tB, *tC, *td;
    int64_t ld_d;
};

// workspace doubles per step: x_{t+1}, tx_{t+1}; the single solve adds gain (2 I) and feed-forward (I)
TPC_GRAD_HD constexpr int slots(int I, bool whole) { return whole ? 4 + 3 * I : 4; }

// An index the optimiser cannot see through (mpc_rollout_newton.hip): re-made per step of the closed loop, so the
// per-lane addresses of the arrays are formed where they are used instead of being held in registers across the loop.
TPC_GRAD_HD int64_t per_step(int64_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(k));
#endif
    return k;
}

// Nothing is scheduled across this point (device only): a group of loads is consumed before the next is issued.
TPC_GRAD_HD void group_end() {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// the model's tangent in direction d of instance k (the fields of Model that carry a tangent; fin = all finite)
template <int I>
TPC_GRAD_HD Model load_tangent(const Dirs& t, int64_t ld, int d, int64_t k) {
    auto in = [&](const double* base, int C, int c) -> double {
        return base ? base[((int64_t)d * C + c) * ld + k] : 0.0;
    };
    Model m;
    m.a00 = in(t.tA, 4, 0); m.a01 = in(t.tA, 4, 1); m.a10 = in(t.tA, 4, 2); m.a11 = in(t.tA, 4, 3);
    m.c0 = in(t.tC, 2, 0); m.c1 = in(t.tC, 2, 1); m.q0 = in(t.tQ, 2, 0); m.q1 = in(t.tQ, 2, 1);
    m.fin = gfinite(m.a00) && gfinite(m.a01) && gfinite(m.a10) && gfinite(m.a11) && gfinite(m.c0) && gfinite(m.c1) &&
            gfinite(m.q0) && gfinite(m.q1);
    m.ok = true;
#pragma unroll
    for (int j = 0; j < I; ++j) {
        m.b0[j] = in(t.tB, 2 * I, j);
        m.b1[j] = in(t.tB, 2 * I, I + j);
        m.r[j] = in(t.tR, I, j);
        m.lo[j] = in(t.tlo, I, j);
        m.hi[j] = in(t.thi, I, j);
        m.fin = m.fin && gfinite(m.b0[j]) && gfinite(m.b1[j]) && gfinite(m.r[j]) && gfinite(m.lo[j]) &&
                gfinite(m.hi[j]);
    }
    return m;
}

// The tangent of one solve from state (xs0, xs1) with state tangent (txs0, txs1): u(t, j), tg(t, c) and ttg(t, c) read
// the recorded controls, the targets and the targets' tangent.  Returns row 0 of tU in tu0; with Whole, out(t, j, v)
// receives every component of tU (row 0 included).  Returns false if a control or a target read is not finite.
template <int I, bool Whole, class U, class TG, class TTG, class OUT>
TPC_GRAD_HD bool step(const Model& m, const Model& tm, int H, double xs0, double xs1, double txs0, double txs1, U u_at,
                      TG tg_at, TTG ttg_at, OUT out, double* ws, int64_t wn, double (&tu0)[2]) {
    auto slot = [&](int q, int t) -> double& { return ws[((int64_t)q * H + t) * wn]; };
    const double a00 = m.a00, a01 = m.a01, a10 = m.a10, a11 = m.a11, c0 = m.c0, c1 = m.c1, q0 = m.q0, q1 = m.q1;
    // ub: the bounds' tangent where u sits on a bound (the branch order of grad::qp_step), 0 on F
    // (both tangents are read before the choice: a choice between two addresses would put the model in private memory)
    auto on_bound = [&](int j, double u) -> double {
        const double tl = tm.lo[j], th = tm.hi[j];
        const double upper = u >= m.hi[j] ? th : 0.0;
        return u <= m.lo[j] ? tl : upper;
    };
    bool fin = true;

    // ---- 1. forward: x_{t+1}, tx_{t+1} -> the step's slots (0, 1: x; 2, 3: tx)
    {
        double x0 = xs0, x1 = xs1, d0 = txs0, d1 = txs1;
        for (int t = 0; t < H; ++t) {
            double y0 = gfma(a00, x0, gfma(a01, x1, c0)), y1 = gfma(a10, x0, gfma(a11, x1, c1));
            double e0 = gfma(tm.a00, x0, gfma(tm.a01, x1, gfma(a00, d0, gfma(a01, d1, tm.c0))));
            double e1 = gfma(tm.a10, x0, gfma(tm.a11, x1, gfma(a10, d0, gfma(a11, d1, tm.c1))));
#pragma unroll
            for (int j = 0; j < I; ++j) {
                const double u = u_at(t, j);
                fin = fin && gfinite(u);
                const double ub = on_bound(j, u);
                y0 = gfma(m.b0[j], u, y0);
                y1 = gfma(m.b1[j], u, y1);
                e0 = gfma(tm.b0[j], u, gfma(m.b0[j], ub, e0));
                e1 = gfma(tm.b1[j], u, gfma(m.b1[j], ub, e1));
            }
            x0 = y0; x1 = y1; d0 = e0; d1 = e1;
            slot(0, t) = x0; slot(1, t) = x1; slot(2, t) = d0; slot(3, t) = d1;
        }
    }

    // ---- 2. backward, t = H-1 .. 0: the costates p_t, tp_t, r_t, and the masked Riccati step with g = r_t.
    // V_{t+1}(dx) = 1/2 dx' P dx + s' dx, P = s = 0 at t + 1 = H.
    double P0 = 0.0, P1 = 0.0, D0 = 0.0, D1 = 0.0;   // p_{t+1}, tp_{t+1}
    double p00 = 0.0, p01 = 0.0, p11 = 0.0, s0 = 0.0, s1 = 0.0;
    double kf[2] = {0.0, 0.0}, ub[2] = {0.0, 0.0};   // of the step last done: t = 0 after the loop
    for (int t = H - 1; t >= 0; --t) {
        const double x0 = slot(0, t), x1 = slot(1, t), d0 = slot(2, t), d1 = slot(3, t);
        const double tg0 = tg_at(t, 0), tg1 = tg_at(t, 1), ttg0 = ttg_at(t, 0), ttg1 = ttg_at(t, 1);
        fin = fin && gfinite(tg0) && gfinite(tg1) && gfinite(ttg0) && gfinite(ttg1);
        const double e0 = x0 - tg0, e1 = x1 - tg1, de0 = d0 - ttg0, de1 = d1 - ttg1;
        const double p0 = gfma(a00, P0, gfma(a10, P1, q0 * e0)), p1 = gfma(a01, P0, gfma(a11, P1, q1 * e1));
        const double dp0 = gfma(tm.a00, P0, gfma(tm.a10, P1, gfma(a00, D0, gfma(a10, D1, gfma(tm.q0, e0, q0 * de0)))));
        const double dp1 = gfma(tm.a01, P0, gfma(tm.a11, P1, gfma(a01, D0, gfma(a11, D1, gfma(tm.q1, e1, q1 * de1)))));
        P0 = p0; P1 = p1; D0 = dp0; D1 = dp1;
        double g[2];
        bool fr[2];
#pragma unroll
        for (int j = 0; j < I; ++j) {
            const double u = u_at(t, j);
            ub[j] = on_bound(j, u);
            fr[j] = !(u <= m.lo[j] || u >= m.hi[j]);
            g[j] = gfma(tm.b0[j], p0, gfma(tm.b1[j], p1, gfma(m.b0[j], dp0, gfma(m.b1[j], dp1,
                                                                                 gfma(tm.r[j], u, m.r[j] * ub[j])))));
        }
        // -- from here to the end of the step: grad::riccati_passes, pass 1, operation for operation
        // S = Q + P (symmetric), SA = S A, SB = S B
        const double S00 = q0 + p00, S01 = p01, S11 = q1 + p11;
        const double SA00 = gfma(S00, a00, S01 * a10), SA01 = gfma(S00, a01, S01 * a11);
        const double SA10 = gfma(S01, a00, S11 * a10), SA11 = gfma(S01, a01, S11 * a11);
        double SB0[2], SB1[2], Hux0[2], Hux1[2], hu[2];
#pragma unroll
        for (int j = 0; j < I; ++j) {
            SB0[j] = gfma(S00, m.b0[j], S01 * m.b1[j]);
            SB1[j] = gfma(S01, m.b0[j], S11 * m.b1[j]);
            // Hux = B' S A (row j), hu = B' s - g; a component that is not free gets a zero row
            Hux0[j] = fr[j] ? gfma(m.b0[j], SA00, m.b1[j] * SA10) : 0.0;
            Hux1[j] = fr[j] ? gfma(m.b0[j], SA01, m.b1[j] * SA11) : 0.0;
            hu[j] = fr[j] ? gfma(m.b0[j], s0, gfma(m.b1[j], s1, -g[j])) : 0.0;
        }
        // Huu = R + B' S B on F; identity on the other components (their solution is then 0)
        double K0[2], K1[2];
        if (I == 1) {
            const double h = fr[0] ? gfma(m.b0[0], SB0[0], gfma(m.b1[0], SB1[0], m.r[0])) : 1.0;
            const double rd = 1.0 / h;
            K0[0] = -(rd * Hux0[0]);
            K1[0] = -(rd * Hux1[0]);
            kf[0] = -(rd * hu[0]);
        } else {
            const bool both = fr[0] && fr[I - 1];
            const double h00 = fr[0] ? gfma(m.b0[0], SB0[0], gfma(m.b1[0], SB1[0], m.r[0])) : 1.0;
            const double h11 =
                fr[I - 1] ? gfma(m.b0[I - 1], SB0[I - 1], gfma(m.b1[I - 1], SB1[I - 1], m.r[I - 1])) : 1.0;
            const double h01 = both ? gfma(m.b0[0], SB0[I - 1], m.b1[0] * SB1[I - 1]) : 0.0;
            const double rd = 1.0 / gfma(h00, h11, -(h01 * h01));
            const double i00 = h11 * rd, i11 = h00 * rd, i01 = -(h01 * rd);
            K0[0] = -gfma(i00, Hux0[0], i01 * Hux0[I - 1]);
            K1[0] = -gfma(i00, Hux1[0], i01 * Hux1[I - 1]);
            kf[0] = -gfma(i00, hu[0], i01 * hu[I - 1]);
            K0[I - 1] = -gfma(i01, Hux0[0], i11 * Hux0[I - 1]);
            K1[I - 1] = -gfma(i01, Hux1[0], i11 * Hux1[I - 1]);
            kf[I - 1] = -gfma(i01, hu[0], i11 * hu[I - 1]);
        }
        // P_t = A' S A + Hux' K,  s_t = A' s + Hux' k
        double n00 = gfma(a00, SA00, a10 * SA10), n01 = gfma(a00, SA01, a10 * SA11), n11 = gfma(a01, SA01, a11 * SA11);
        double m0 = gfma(a00, s0, a10 * s1), m1 = gfma(a01, s0, a11 * s1);
#pragma unroll
        for (int j = 0; j < I; ++j) {
            n00 = gfma(Hux0[j], K0[j], n00);
            n01 = gfma(Hux0[j], K1[j], n01);
            n11 = gfma(Hux1[j], K1[j], n11);
            m0 = gfma(Hux0[j], kf[j], m0);
            m1 = gfma(Hux1[j], kf[j], m1);
            if (Whole) {
                slot(4 + 2 * j, t) = K0[j];
                slot(4 + 2 * j + 1, t) = K1[j];
                slot(4 + 2 * I + j, t) = kf[j];
            }
        }
        p00 = n00; p01 = n01; p11 = n11; s0 = m0; s1 = m1;
    }
    // row 0: dx_0 = 0, so w_0 is the feed-forward of step 0
#pragma unroll
    for (int j = 0; j < I; ++j) tu0[j] = ub[j] - kf[j];

    // ---- 3. (the whole sequence) forward: w_t = K_t dx_t + k_t, tU_t = ub_t - w_t
    if (Whole) {
        double d0 = 0.0, d1 = 0.0;
        for (int t = 0; t < H; ++t) {
            double w[2];
            double e0 = gfma(a00, d0, a01 * d1), e1 = gfma(a10, d0, a11 * d1);
#pragma unroll
            for (int j = 0; j < I; ++j) {
                w[j] = gfma(slot(4 + 2 * j, t), d0, gfma(slot(4 + 2 * j + 1, t), d1, slot(4 + 2 * I + j, t)));
                out(t, j, on_bound(j, u_at(t, j)) - w[j]);
            }
#pragma unroll
            for (int j = 0; j < I; ++j) {
                e0 = gfma(m.b0[j], w[j], e0);
                e1 = gfma(m.b1[j], w[j], e1);
            }
            d0 = e0; d1 = e1;
        }
    }
    return fin;
}

// Direction d of instance k of the single solve.  ws points at the lane's first workspace element.  Returns the
// TPC_MPC_FLAG_* bits (0x1 non-finite, 0x4 bad model); a flagged (d, k) pair gets an all-zero tu block.
template <int I>
TPC_GRAD_HD uint32_t instance(const Args& a, int H, int d, int64_t k, double* ws, int64_t wn) {
    const int64_t ld = a.ld;
    auto in = [&](const double* base, int c) -> double { return base[(int64_t)c * ld + k]; };
    auto tin = [&](const double* base, int C, int c) -> double {
        return base ? base[((int64_t)d * C + c) * ld + k] : 0.0;
    };
    const Model m = load_model<I>(a.A, a.B, a.C, a.Q, a.R, a.lo, a.hi, ld, k);
    const Model tm = load_tangent<I>(a.t, ld, d, k);
    const double xs0 = in(a.x0, 0), xs1 = in(a.x0, 1), txs0 = tin(a.t.tx0, 2, 0), txs1 = tin(a.t.tx0, 2, 1);
    bool fin = m.fin && tm.fin && gfinite(xs0) && gfinite(xs1) && gfinite(txs0) && gfinite(txs1);
    double* tu = a.tu + ((int64_t)d * H * I) * ld + k;
    double tu0[2];
    fin = step<I, true>(
              m, tm, H, xs0, xs1, txs0, txs1, [&](int t, int j) { return in(a.u, t * I + j); },
              [&](int t, int c) { return in(a.targets, 2 * t + c); },
              [&](int t, int c) { return tin(a.t.ttargets, 2 * H, 2 * t + c); },
              [&](int t, int j, double v) { tu[(int64_t)(t * I + j) * ld] = v; }, ws, wn, tu0) && fin;
    const uint32_t flags = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    if (flags)
        for (int c = 0; c < H * I; ++c) tu[(int64_t)c * ld] = 0.0;
    return flags;
}

// Direction d of instance k of the closed loop: the sweep over the steps (include/tpc_mpc.h, tpc_mpc_rollout_forward).
// Step kk solves from x_kk (x0, then the recorded states[kk-1]) with the targets T_kk of grad::rollout_instance's map;
// tT_kk comes from ttargets / tnlt through the same map.  tx_kk is carried from step to step in registers; the
// workspace is reused by every step.  With Plant (tpc_mpc_rollout_plant_forward) the state's tangent moves with pl's
// arrays and tangents: they are read at the step's last line and not held across the horizon passes.
template <int I, bool Plant = false>
TPC_GRAD_HD uint32_t rollout_instance(const RollArgs& a, int H, int d, int64_t k0, double* ws0, int64_t wn,
                                      const RollPlant* pl = nullptr) {
    const int64_t ld = a.ld;
    const int S = a.steps;
    const int HI = H * I;
    int64_t k = k0;
    auto in = [&](const double* base, int64_t c) -> double { return base[c * ld + k]; };
    auto tin = [&](const double* base, int64_t C, int64_t c) -> double {
        return base ? base[((int64_t)d * C + c) * ld + k] : 0.0;
    };
    const Model m = load_model<I>(a.A, a.B, a.C, a.Q, a.R, a.lo, a.hi, ld, k);
    const Model tm = load_tangent<I>(a.t, ld, d, k);
    double tx0 = tin(a.t.tx0, 2, 0), tx1 = tin(a.t.tx0, 2, 1);   // tx_kk
    bool fin = m.fin && tm.fin && gfinite(tx0) && gfinite(tx1) && gfinite(in(a.states, 2 * (int64_t)S - 2)) &&
               gfinite(in(a.states, 2 * (int64_t)S - 1));
    const int64_t urow = (int64_t)d * S * I, xrow = (int64_t)d * S * 2;   // the direction's blocks of tu and tx

    for (int kk = 0; kk < S; ++kk) {
        k = per_step(k0);
        double* ws = ws0 + (k - k0);
        const double xs0 = kk == 0 ? in(a.x0, 0) : in(a.states, 2 * (int64_t)kk - 2);
        const double xs1 = kk == 0 ? in(a.x0, 1) : in(a.states, 2 * (int64_t)kk - 1);
        fin = fin && gfinite(xs0) && gfinite(xs1);
        const int64_t sq = (int64_t)kk * HI;   // first row of U_kk
        // the target map of step kk: component c of T_kk[t] as (0: targets, 1: new_last_targets; component index)
        auto tmap = [&](int t, int c, int* which) -> int64_t {
            const int r = t + kk;
            if (r <= H - 1) { *which = 0; return 2 * r + c; }
            if (a.nlt) { *which = 1; return 2 * (int64_t)(r - (H - 1)) + c; }
            *which = 0;
            return 2 * (H - 1) + c;
        };
        double tu0[2];
        fin = step<I, false>(
                  m, tm, H, xs0, xs1, tx0, tx1, [&](int t, int j) { return in(a.seq, sq + t * I + j); },
                  [&](int t, int c) {
                      int w;
                      const int64_t i = tmap(t, c, &w);
                      return in(w ? a.nlt : a.targets, i);
                  },
                  [&](int t, int c) {
                      int w;
                      const int64_t i = tmap(t, c, &w);
                      return w ? tin(a.t.tnlt, 2 * (int64_t)S, i) : tin(a.t.ttargets, 2 * H, i);
                  },
                  [](int, int, double) {}, ws, wn, tu0) && fin;
        if (Plant) {   // the same line on the plant's values, then the disturbance's tangent
            // (read in three groups, the index re-made before each: the values' addresses are formed where they are
            // used and no group is held while the next is read, so the lane stays in its parent's occupancy bracket)
            // a null tangent is zero: the read goes to the primal array instead and its value is dropped, so that the
            // plant line holds no branch (a branch per array costs the lane its parent's occupancy)
            // (the direction is re-made opaque like the index: its row offsets are per lane and would be held too)
            int64_t dq = d;
            auto ptin = [&](const double* t, const double* primal, int64_t C, int64_t c) -> double {
                const double* b = t ? t : primal;
                const double v = b[((t ? dq : 0) * C + c) * ld + k];
                return t ? v : 0.0;
            };
            k = per_step(k0);
            dq = per_step(d);
            const double tc0 = ptin(pl->tC, pl->C, 2, 0), tc1 = ptin(pl->tC, pl->C, 2, 1);
            const double A00 = in(pl->A, 0), A01 = in(pl->A, 1), A10 = in(pl->A, 2), A11 = in(pl->A, 3);
            fin = fin && gfinite(A00) && gfinite(A01) && gfinite(A10) && gfinite(A11) && gfinite(tc0) && gfinite(tc1) &&
                  gfinite(in(pl->C, 0)) && gfinite(in(pl->C, 1));
            double y0 = gfma(A00, tx0, gfma(A01, tx1, tc0));
            double y1 = gfma(A10, tx0, gfma(A11, tx1, tc1));
            group_end();
            k = per_step(k0);
            dq = per_step(d);
            const double T00 = ptin(pl->tA, pl->A, 4, 0), T01 = ptin(pl->tA, pl->A, 4, 1);
            const double T10 = ptin(pl->tA, pl->A, 4, 2), T11 = ptin(pl->tA, pl->A, 4, 3);
            fin = fin && gfinite(T00) && gfinite(T01) && gfinite(T10) && gfinite(T11);
            y0 = gfma(T00, xs0, gfma(T01, xs1, y0));
            y1 = gfma(T10, xs0, gfma(T11, xs1, y1));
            group_end();
            k = per_step(k0);
            dq = per_step(d);
#pragma unroll
            for (int j = 0; j < I; ++j) {
                const double u0 = in(a.seq, sq + j);
                const double b0 = in(pl->B, j), b1 = in(pl->B, I + j);
                const double tb0 = ptin(pl->tB, pl->B, 2 * I, j), tb1 = ptin(pl->tB, pl->B, 2 * I, I + j);
                fin = fin && gfinite(b0) && gfinite(b1) && gfinite(tb0) && gfinite(tb1);
                y0 = gfma(tb0, u0, gfma(b0, tu0[j], y0));
                y1 = gfma(tb1, u0, gfma(b1, tu0[j], y1));
                a.tu[(urow + (int64_t)kk * I + j) * ld + k] = tu0[j];
            }
            if (pl->td) {
                const double* td = pl->td + (dq * 2 * S + 2 * (int64_t)kk) * pl->ld_d + k;
                const double e0 = td[0], e1 = td[pl->ld_d];
                fin = fin && gfinite(e0) && gfinite(e1);
                y0 = y0 + e0;
                y1 = y1 + e1;
            }
            tx0 = y0; tx1 = y1;
            if (a.tx) {
                a.tx[(xrow + 2 * (int64_t)kk) * ld + k] = tx0;
                a.tx[(xrow + 2 * (int64_t)kk + 1) * ld + k] = tx1;
            }
            continue;
        }
        // the plant's tangent: tx_{kk+1} = tA x + A tx + tB u0 + B tu0 + tC
        double y0 = gfma(tm.a00, xs0, gfma(tm.a01, xs1, gfma(m.a00, tx0, gfma(m.a01, tx1, tm.c0))));
        double y1 = gfma(tm.a10, xs0, gfma(tm.a11, xs1, gfma(m.a10, tx0, gfma(m.a11, tx1, tm.c1))));
#pragma unroll
        for (int j = 0; j < I; ++j) {
            const double u0 = in(a.seq, sq + j);
            y0 = gfma(tm.b0[j], u0, gfma(m.b0[j], tu0[j], y0));
            y1 = gfma(tm.b1[j], u0, gfma(m.b1[j], tu0[j], y1));
            a.tu[(urow + (int64_t)kk * I + j) * ld + k] = tu0[j];
        }
        tx0 = y0; tx1 = y1;
        if (a.tx) {
            a.tx[(xrow + 2 * (int64_t)kk) * ld + k] = tx0;
            a.tx[(xrow + 2 * (int64_t)kk + 1) * ld + k] = tx1;
        }
    }

    k = per_step(k0);
    const uint32_t flags = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    if (flags) {
        for (int64_t c = 0; c < (int64_t)S * I; ++c) a.tu[(urow + c) * ld + k] = 0.0;
        if (a.tx)
            for (int64_t c = 0; c < 2 * (int64_t)S; ++c) a.tx[(xrow + c) * ld + k] = 0.0;
    }
    return flags;
}

}  // namespace tangent
}  // namespace tpc
