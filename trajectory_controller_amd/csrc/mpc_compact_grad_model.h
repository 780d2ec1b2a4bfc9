// Backward pass of the exact compact solve (tpc_mpc_solve_batch_compact_exact_backward, include/tpc_mpc.h): the
// arithmetic of ONE instance, shared by the gfx950 kernels (mpc_compact_grad.hip) and the host path of the same entry.
// It is grad::qp_step<2> (mpc_grad_model.h), as it is, on the model cexact::build_model (mpc_newton_compact_model.h)
// makes from v in registers -- C = 0, x0 = 0, every target (dy, dphi) -- followed by the chain rule of that model
// building, folded in registers:
//   a01 = b0[1] = Tv, b1[0] = Tv / l, b1[1] = -(Tv / l), Tv = T * v, so with S = dA01 + dB0[1], D = dB1[0] - dB1[1]
//   dv = T S + (T / l) D        dT = v S + (v / l) D        dl = -((Tv / l) / l) D
//   d(dy), d(dphi) = the sums of dL/dtarget_t over the steps, Q, R and the bounds pass through.
// No model, target or gradient row of the general form is read or written: 3 + 2H doubles and the incoming gradient in,
// three doubles (and the optional rows) out.  The per-step values go through one pointer, ws[(q * H + t) * wn], as in
// mpc_newton_compact_model.h: the handle's gradient workspace, or with a compile-time horizon an array of the lane's own.
// Every operation of the chain rule is rounded on its own (-ffp-contract=off; fused operations are written gfma), so
// kernels and host path give the same bits, and both equal tpc_mpc_solve_batch_general_backward on the expanded arrays
// pushed through the same lines (tests/test_compact_grad_host.py).
#pragma once

#include "mpc_newton_compact_model.h"

namespace tpc {
namespace cgrad {

using grad::gfinite;

constexpr int kI = 2;
constexpr int kSlots = grad::slots(kI);   // workspace doubles per step
constexpr int kParams = 10;               // weight_y, weight_phi, weight_steering_front, weight_steering_rear,
                                          // step_size, wheelbase, lower[0], lower[1], upper[0], upper[1]

// v, dy, dphi [n], seq [H*2] rows ld apart, status [n] (may be null); the incoming gradient: gf, gr [n], gs [H*2] rows
// ld apart (any may be null: zero); the outputs (any may be null): dv, ddy, ddphi, kkt [n], rows [10] rows ld apart
struct Args {
    int64_t n, ld;
    const double *v, *dy, *dphi, *seq;
    const int32_t* status;
    const double *gf, *gr, *gs;
    double T, l, q0, q1, r[2], lo[2], hi[2];   // tpc_mpc_params: step_size, wheelbase, weights, bounds
    const double* params;   // the rows entry: [10] rows ld apart, instance k's own ten values in column k, in the order
                            // of kParams; the ten fields above are unused
    double *dv, *ddy, *ddphi, *rows, *kkt;
};

// One instance.  HC > 0: the horizon, at compile time (Hrt is ignored); HC == 0: Hrt.  ws points at the instance's
// first workspace element.  Writes the instance's outputs and leaves its ten shared-parameter gradients in row (zeros
// for an excluded instance).  Returns its TPC_MPC_FLAG_* bits (0x1 non-finite, 0x4 bad model); a negative status
// excludes the instance without a flag of its own.
// ROWS: the model, T and l are instance k's own (a.params), and row is the gradient with respect to them.
template <int HC, bool ROWS = false>
TPC_GRAD_HD uint32_t compact_grad_instance(const Args& a, int Hrt, int64_t k, double* ws, int64_t wn,
                                           double (&row)[kParams]) {
    constexpr int I = kI;
    const int H = HC > 0 ? HC : Hrt;
    const int64_t ld = a.ld;
    const double v = a.v[k], tg0 = a.dy[k], tg1 = a.dphi[k];
    cexact::Args ma = {};
    if (ROWS) {
        ma.params = a.params; ma.ld_params = ld;
        ma = cexact::instance_params<true>(ma, k);
    } else {
        ma.T = a.T; ma.l = a.l; ma.q0 = a.q0; ma.q1 = a.q1;
#pragma unroll
        for (int j = 0; j < I; ++j) { ma.r[j] = a.r[j]; ma.lo[j] = a.lo[j]; ma.hi[j] = a.hi[j]; }
    }
    const double T = ma.T, l = ma.l;
    const grad::Model m = cexact::build_model(ma, v);
    const double gf = a.gf ? a.gf[k] : 0.0, gr = a.gr ? a.gr[k] : 0.0;

    grad::Sums s;
    double sa = 0.0, sb = 0.0, dx00, dx01;
    const bool fin = grad::qp_step<I>(
                         m, H, 0.0, 0.0, [&](int t, int j) { return a.seq[(int64_t)(t * I + j) * ld + k]; },
                         [&](int t, int j) {
                             const double gs = a.gs ? a.gs[(int64_t)(t * I + j) * ld + k] : 0.0;
                             return t == 0 ? gs + (j == 0 ? gf : gr) : gs;
                         },
                         [&](int, int c) { return c == 0 ? tg0 : tg1; },
                         [&](int, double v0, double v1) { sa = sa + v0; sb = sb + v1; }, ws, wn, s, dx00, dx01) &&
                     m.fin && (!ROWS || (gfinite(T) && gfinite(l)));   // as cexact::exact_instance decides it

    const uint32_t flags = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    const bool zero = flags != 0u || (a.status && a.status[k] < 0);

    // the chain rule of build_model
    const double S = s.A01 + s.B0[1], D = s.B1[0] - s.B1[1], Tv = T * v;
    const double dv = T * S + (T / l) * D;
    row[0] = s.Q0; row[1] = s.Q1; row[2] = s.R[0]; row[3] = s.R[1];
    row[4] = v * S + (v / l) * D;
    row[5] = -((Tv / l) / l) * D;
    row[6] = s.lo[0]; row[7] = s.lo[1]; row[8] = s.hi[0]; row[9] = s.hi[1];
#pragma unroll
    for (int c = 0; c < kParams; ++c) row[c] = zero ? 0.0 : row[c];

    if (a.dv) a.dv[k] = zero ? 0.0 : dv;
    if (a.ddy) a.ddy[k] = zero ? 0.0 : sa;
    if (a.ddphi) a.ddphi[k] = zero ? 0.0 : sb;
    if (a.kkt) a.kkt[k] = zero ? 0.0 : s.kkt;
    if (a.rows)
#pragma unroll
        for (int c = 0; c < kParams; ++c) a.rows[(int64_t)c * ld + k] = row[c];
    return flags;
}

}  // namespace cgrad
}  // namespace tpc
