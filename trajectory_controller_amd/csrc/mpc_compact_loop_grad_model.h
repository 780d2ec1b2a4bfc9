// Backward pass of the compact closed loop (tpc_mpc_rollout_compact_exact_backward, include/tpc_mpc.h): the arithmetic
// of ONE instance, shared by the gfx950 kernels (mpc_compact_loop_grad.hip) and the host path of the same entry.  It is
// the reverse sweep over the steps of grad::rollout_instance<2, false> (mpc_grad_model.h), operation for operation, with
// no new last targets, on the model cexact::build_model (mpc_newton_compact_model.h) makes from v in registers -- C = 0,
// every target (dy, dphi) at every step, x0 the call's column or (+0.0, +0.0) -- followed by the chain rule of that
// model building as cgrad::compact_grad_instance (mpc_compact_grad_model.h) folds it, on the sums of ALL steps:
//   for kk = S-1 .. 0:  mu = lambda + grad_states[kk];  the plant terms of x_{kk+1} = A x_kk + B u0_kk into the sums;
//                       g0 = B' mu + grad_controls[kk];  grad::qp_step<2>, unchanged, at (x_kk, U_kk, g0 on row 0);
//                       lambda = A' mu + dL/dx_kk of the solve
//   dx0 = lambda;  ddelta_y, ddelta_phi = the sums of every dL/dtarget, in the order qp_step hands them over (kk
//   descending, t descending inside a step), each addition rounded on its own;  dv, rows[0..9] by the chain rule.
// x_kk is x0 or the recorded states[kk-1]: the state is never recomputed.  lambda, the sums and the two target sums live
// in registers (v, the target and x0 are re-read where they are used); the per-step Riccati slots, ws[(q * H + t) * wn] as in mpc_compact_grad_model.h, are reused by every
// step.  No model, target or gradient row of the general form is read or written.
// Every operation is rounded on its own (-ffp-contract=off; fused operations are written gfma), so kernels and host path
// give the same bits, and both equal tpc_mpc_rollout_backward on the expanded arrays pushed through the same lines
// (tests/test_compact_loop_grad_host.py).
#pragma once

#include "mpc_newton_compact_model.h"

namespace tpc {
namespace cloopgrad {

using grad::gfinite;
using grad::gfma;
using polish::per_step;   // the step loop costs no registers beyond one step's

constexpr int kI = 2;
constexpr int kSlots = grad::slots(kI);   // workspace doubles per horizon step
constexpr int kParams = 10;               // the order of cgrad::kParams

// v, dy, dphi [n], x0 [2] (may be null: zeros), seq [S*H*2], states [S*2], status [S] (int32, may be null), the incoming
// gradient gu [S*2], gx [S*2] (either may be null: zero), all rows ld apart; the outputs (any may be null): dv, ddy,
// ddphi, kkt [n], dx0 [2] and rows [10] rows ld apart
struct Args {
    int64_t n, ld;
    int32_t steps;
    const double *v, *dy, *dphi, *x0, *seq, *states;
    const int32_t* status;
    const double *gu, *gx;
    double T, l, q0, q1, r[2], lo[2], hi[2];   // tpc_mpc_params: step_size, wheelbase, weights, bounds
    double *dv, *ddy, *ddphi, *dx0, *rows, *kkt;
};

// One instance, every step.  HC > 0: the horizon, at compile time (Hrt is ignored; ws0 is then an array of the lane's
// own, wn == 1, whose every index is a constant); HC == 0: Hrt.  ws0 points at the instance's first workspace element.
// Writes the instance's outputs and leaves its ten shared-parameter gradients in row (zeros for an excluded instance).
// Returns its TPC_MPC_FLAG_* bits (0x1 non-finite, 0x4 bad model); a negative status at any step excludes the instance
// without a flag of its own.
template <int HC>
TPC_GRAD_HD uint32_t loop_grad_instance(const Args& a, int Hrt, int64_t k0, double* ws0, int64_t wn,
                                        double (&row)[kParams]) {
    constexpr int I = kI;
    const int H = HC > 0 ? HC : Hrt, S = a.steps;
    const int HI = H * I;
    const int64_t ld = a.ld;
    double* ws = ws0;
    cexact::Args ma = {};
    ma.T = a.T; ma.l = a.l; ma.q0 = a.q0; ma.q1 = a.q1;
#pragma unroll
    for (int j = 0; j < I; ++j) { ma.r[j] = a.r[j]; ma.lo[j] = a.lo[j]; ma.hi[j] = a.hi[j]; }
    const double T = ma.T, l = ma.l;
    const grad::Model m = cexact::build_model(ma, a.v[k0]);
    // (x0's finiteness is step 0's test of x_kk below: the same AND)
    bool fin = m.fin && gfinite(a.states[(2 * (int64_t)S - 2) * ld + k0]) &&
               gfinite(a.states[(2 * (int64_t)S - 1) * ld + k0]);
    bool stopped = false;   // a negative status at any step

    grad::Sums s;
    double sa = 0.0, sb = 0.0;
    double l0 = 0.0, l1 = 0.0;   // lambda = dL/dx_{kk+1} from the steps after kk
    for (int kk = S - 1; kk >= 0; --kk) {
        const int64_t k = per_step(k0);
        if (HC == 0) ws = ws0 + (k - k0);
        auto in = [&](const double* base, int64_t c) -> double { return base[c * ld + k]; };
        // v, the target and x0 are read where they are used, not held across the steps: at H = 5 the register kernel
        // has no VGPR to spare
        if (a.status) stopped = stopped || a.status[(int64_t)kk * ld + k] < 0;
        const double gx0 = a.gx ? in(a.gx, 2 * (int64_t)kk) : 0.0, gx1 = a.gx ? in(a.gx, 2 * (int64_t)kk + 1) : 0.0;
        const double mu0 = l0 + gx0, mu1 = l1 + gx1;   // total dL/dx_{kk+1}
        const double xs0 = kk == 0 ? (a.x0 ? in(a.x0, 0) : 0.0) : in(a.states, 2 * (int64_t)kk - 2);
        const double xs1 = kk == 0 ? (a.x0 ? in(a.x0, 1) : 0.0) : in(a.states, 2 * (int64_t)kk - 1);
        fin = fin && gfinite(gx0) && gfinite(gx1) && gfinite(xs0) && gfinite(xs1);
        const int64_t sq = (int64_t)kk * HI;   // first row of U_kk
        // the plant update x_{kk+1} = A x_kk + B u0_kk + C: its terms go into the sums
        double g0[2];   // dL/du0_kk = G_u[kk] + B' mu
        s.A00 = gfma(mu0, xs0, s.A00);
        s.A01 = gfma(mu0, xs1, s.A01);
        s.A10 = gfma(mu1, xs0, s.A10);
        s.A11 = gfma(mu1, xs1, s.A11);
        s.C0 = s.C0 + mu0;
        s.C1 = s.C1 + mu1;
#pragma unroll
        for (int j = 0; j < I; ++j) {
            const double u0 = in(a.seq, sq + j);
            const double gu = a.gu ? in(a.gu, (int64_t)kk * I + j) : 0.0;
            fin = fin && gfinite(gu);
            s.B0[j] = gfma(mu0, u0, s.B0[j]);
            s.B1[j] = gfma(mu1, u0, s.B1[j]);
            g0[j] = gfma(m.b0[j], mu0, gfma(m.b1[j], mu1, gu));
        }
        double dx00, dx01;
        fin = grad::qp_step<I>(
                  m, H, xs0, xs1, [&](int t, int j) { return in(a.seq, sq + t * I + j); },
                  [&](int t, int j) { return t == 0 ? g0[j] : 0.0; },
                  [&](int, int c) { return c == 0 ? a.dy[k] : a.dphi[k]; },
                  [&](int, double v0, double v1) { sa = sa + v0; sb = sb + v1; }, ws, wn, s, dx00, dx01) && fin;
        // lambda_kk = A' mu + dL/dx_kk of the solve
        l0 = gfma(m.a00, mu0, gfma(m.a10, mu1, dx00));
        l1 = gfma(m.a01, mu0, gfma(m.a11, mu1, dx01));
    }

    const int64_t k = per_step(k0);
    const double v = a.v[k];
    const uint32_t flags = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    const bool zero = flags != 0u || stopped;

    // the chain rule of build_model, as cgrad::compact_grad_instance has it
    const double Sm = s.A01 + s.B0[1], D = s.B1[0] - s.B1[1], Tv = T * v;
    const double dv = T * Sm + (T / l) * D;
    row[0] = s.Q0; row[1] = s.Q1; row[2] = s.R[0]; row[3] = s.R[1];
    row[4] = v * Sm + (v / l) * D;
    row[5] = -((Tv / l) / l) * D;
    row[6] = s.lo[0]; row[7] = s.lo[1]; row[8] = s.hi[0]; row[9] = s.hi[1];
#pragma unroll
    for (int c = 0; c < kParams; ++c) row[c] = zero ? 0.0 : row[c];

    if (a.dv) a.dv[k] = zero ? 0.0 : dv;
    if (a.ddy) a.ddy[k] = zero ? 0.0 : sa;
    if (a.ddphi) a.ddphi[k] = zero ? 0.0 : sb;
    if (a.kkt) a.kkt[k] = zero ? 0.0 : s.kkt;
    if (a.dx0) {
        a.dx0[k] = zero ? 0.0 : l0;
        a.dx0[ld + k] = zero ? 0.0 : l1;
    }
    if (a.rows)
#pragma unroll
        for (int c = 0; c < kParams; ++c) a.rows[(int64_t)c * ld + k] = row[c];
    return flags;
}

}  // namespace cloopgrad
}  // namespace tpc
