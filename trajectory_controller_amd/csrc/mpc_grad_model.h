// Backward pass of the general form (tpc_mpc_solve_batch_general_backward, include/tpc_mpc.h): the arithmetic of ONE
// instance, shared by the gfx950 kernel (mpc_grad.hip) and the host path of the same entry.  Every fused operation is an
// explicit fma() and the translation unit is built with -ffp-contract=off, so the kernel and the host path give the same
// bits (tests/test_grad_gpu.py holds them to it).
//
// The model is dlib's (mpc.h:255-283): x_0 = x0, x_{t+1} = A x_t + B u_t + C, cost
//   sum_t 1/2 (x_{t+1} - target_t)' Q (x_{t+1} - target_t) + 1/2 u_t' R u_t,
// gradient df_t = B' p_t + R u_t with the costate p_t = sum_{s>=t} (A')^(s-t) Q (x_{s+1} - target_s).
// A component (t, j) is active iff u <= lower_j or u >= upper_j; F is the rest.  Given dL/du = g, the adjoint direction
// w = H_FF^-1 g_F (w_A = 0) minimises 1/2 w'Hw - g'w with w_A fixed to 0: an LQR problem on the 2-state response
// dx (dx_0 = 0, dx_{t+1} = A dx_t + B w_t) with at most a 2x2 input block per step, solved by a masked Riccati sweep.
// Then, with dp the costate of Q dx and e_{s+1} = x_{s+1} - target_s:
//   dL/dtarget_s = Q dx_{s+1}          dL/dQ = -sum e (.) dx         dL/dR = -sum w (.) u
//   dL/dx0 = -A' dp_0                  dL/dC = -sum dp_t
//   dL/dB = -sum (dp_t u_t' + p_t w_t')   dL/dA = -sum (dp_t x_t' + p_t dx_t')
//   dL/dlower_j (dL/dupper_j) = sum over the steps where (t, j) is active on that bound of (g - H w)_{t,j},
//   (H w)_t = B' dp_t + R w_t.
//
// Three passes over the horizon, no per-step array in registers or private memory (a private array indexed by the step
// lands in scratch): the per-step quantities live in a workspace of kSlots(I) doubles per step, element (q, t) of
// instance k at ws[(q * H + t) * wn + k] -- neighbouring instances at neighbouring addresses.
//   1. backward: the Riccati sweep; stores the gain K_t (I x 2) and feed-forward k_t (I) of every step.
//   2. forward:  x_t from u, w_t = K_t dx_t + k_t, dx_t; overwrites step t's slots with x_t, dx_t, w_t.
//   3. backward: p_t, dp_t and every gradient.
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define TPC_GRAD_HD __host__ __device__ inline
#else
#define TPC_GRAD_HD inline
#endif

namespace tpc {
namespace grad {

// SoA arrays, fp64, component c of instance k at base[c * ld + k] (the io's shapes; outputs may be null)
struct Args {
    int64_t n, ld;
    const double *A, *B, *C, *Q, *R, *lo, *hi, *x0, *targets, *u, *g;
    double *dA, *dB, *dC, *dQ, *dR, *dlo, *dhi, *dx0, *dtargets, *kkt;
};

// workspace doubles per step: gain + feed-forward (3 I) in pass 1, x, dx, w (4 + I) from pass 2 on
TPC_GRAD_HD constexpr int slots(int I) { return 4 + I; }

TPC_GRAD_HD double gfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
TPC_GRAD_HD double gabs(double x) { return __builtin_fabs(x); }
TPC_GRAD_HD bool gfinite(double x) { return gabs(x) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// One instance.  ws points at the instance's first workspace element (ws[(q * H + t) * wn]).  Returns its
// TPC_MPC_FLAG_* bits (0x1 non-finite, 0x4 bad model); a flagged instance gets all-zero outputs.
template <int I>
TPC_GRAD_HD uint32_t instance(const Args& a, int H, int64_t k, double* ws, int64_t wn) {
    const int64_t ld = a.ld;
    auto in = [&](const double* base, int c) -> double { return base[(int64_t)c * ld + k]; };
    auto slot = [&](int q, int t) -> double& { return ws[((int64_t)q * H + t) * wn]; };

    const double a00 = in(a.A, 0), a01 = in(a.A, 1), a10 = in(a.A, 2), a11 = in(a.A, 3);
    const double c0 = in(a.C, 0), c1 = in(a.C, 1), q0 = in(a.Q, 0), q1 = in(a.Q, 1);
    double b0[2], b1[2], r[2], lo[2], hi[2];   // row 0 / row 1 of B, per input (constant indices only)
    bool fin = gfinite(a00) && gfinite(a01) && gfinite(a10) && gfinite(a11) && gfinite(c0) && gfinite(c1) &&
               gfinite(q0) && gfinite(q1) && gfinite(in(a.x0, 0)) && gfinite(in(a.x0, 1));
    bool ok = q0 >= 0.0 && q1 >= 0.0;
#pragma unroll
    for (int j = 0; j < I; ++j) {
        b0[j] = in(a.B, j);
        b1[j] = in(a.B, I + j);
        r[j] = in(a.R, j);
        lo[j] = in(a.lo, j);
        hi[j] = in(a.hi, j);
        fin = fin && gfinite(b0[j]) && gfinite(b1[j]) && gfinite(r[j]) && lo[j] == lo[j] && hi[j] == hi[j];
        ok = ok && r[j] > 0.0 && hi[j] >= lo[j];
    }

    // ---- 1. masked Riccati sweep, t = H-1 .. 0.  V_{t+1}(dx) = 1/2 dx' P dx + s' dx, P = s = 0 at t + 1 = H.
    double p00 = 0.0, p01 = 0.0, p11 = 0.0, s0 = 0.0, s1 = 0.0;
    for (int t = H - 1; t >= 0; --t) {
        double u[2], g[2];
        bool fr[2];
#pragma unroll
        for (int j = 0; j < I; ++j) {
            u[j] = in(a.u, t * I + j);
            g[j] = in(a.g, t * I + j);
            fin = fin && gfinite(u[j]) && gfinite(g[j]);
            fr[j] = !(u[j] <= lo[j] || u[j] >= hi[j]);
        }
        // S = Q + P (symmetric), SA = S A, SB = S B
        const double S00 = q0 + p00, S01 = p01, S11 = q1 + p11;
        const double SA00 = gfma(S00, a00, S01 * a10), SA01 = gfma(S00, a01, S01 * a11);
        const double SA10 = gfma(S01, a00, S11 * a10), SA11 = gfma(S01, a01, S11 * a11);
        double SB0[2], SB1[2], Hux0[2], Hux1[2], hu[2];
#pragma unroll
        for (int j = 0; j < I; ++j) {
            SB0[j] = gfma(S00, b0[j], S01 * b1[j]);
            SB1[j] = gfma(S01, b0[j], S11 * b1[j]);
            // Hux = B' S A (row j), hu = B' s - g; a component that is not free gets a zero row
            Hux0[j] = fr[j] ? gfma(b0[j], SA00, b1[j] * SA10) : 0.0;
            Hux1[j] = fr[j] ? gfma(b0[j], SA01, b1[j] * SA11) : 0.0;
            hu[j] = fr[j] ? gfma(b0[j], s0, gfma(b1[j], s1, -g[j])) : 0.0;
        }
        // Huu = R + B' S B on F; identity on the other components (their solution is then 0)
        double K0[2], K1[2], kf[2];
        if (I == 1) {
            const double h = fr[0] ? gfma(b0[0], SB0[0], gfma(b1[0], SB1[0], r[0])) : 1.0;
            const double rd = 1.0 / h;
            K0[0] = -(rd * Hux0[0]);
            K1[0] = -(rd * Hux1[0]);
            kf[0] = -(rd * hu[0]);
        } else {
            const bool both = fr[0] && fr[I - 1];
            const double h00 = fr[0] ? gfma(b0[0], SB0[0], gfma(b1[0], SB1[0], r[0])) : 1.0;
            const double h11 = fr[I - 1] ? gfma(b0[I - 1], SB0[I - 1], gfma(b1[I - 1], SB1[I - 1], r[I - 1])) : 1.0;
            const double h01 = both ? gfma(b0[0], SB0[I - 1], b1[0] * SB1[I - 1]) : 0.0;
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
            slot(2 * j, t) = K0[j];
            slot(2 * j + 1, t) = K1[j];
            slot(2 * I + j, t) = kf[j];
        }
        p00 = n00; p01 = n01; p11 = n11; s0 = m0; s1 = m1;
    }

    // ---- 2. forward: x_t, dx_t, w_t -> the step's slots (0, 1: x; 2, 3: dx; 4..: w)
    double x0 = in(a.x0, 0), x1 = in(a.x0, 1), d0 = 0.0, d1 = 0.0;
    for (int t = 0; t < H; ++t) {
        double w[2], u[2];
#pragma unroll
        for (int j = 0; j < I; ++j) {
            w[j] = gfma(slot(2 * j, t), d0, gfma(slot(2 * j + 1, t), d1, slot(2 * I + j, t)));
            u[j] = in(a.u, t * I + j);
        }
        slot(0, t) = x0; slot(1, t) = x1; slot(2, t) = d0; slot(3, t) = d1;
#pragma unroll
        for (int j = 0; j < I; ++j) slot(4 + j, t) = w[j];
        double y0 = gfma(a00, x0, gfma(a01, x1, c0)), y1 = gfma(a10, x0, gfma(a11, x1, c1));
        double e0 = gfma(a00, d0, a01 * d1), e1 = gfma(a10, d0, a11 * d1);
#pragma unroll
        for (int j = 0; j < I; ++j) {
            y0 = gfma(b0[j], u[j], y0);
            y1 = gfma(b1[j], u[j], y1);
            e0 = gfma(b0[j], w[j], e0);
            e1 = gfma(b1[j], w[j], e1);
        }
        x0 = y0; x1 = y1; d0 = e0; d1 = e1;
    }

    // ---- 3. backward: costates and gradients.  (x0, x1, d0, d1) hold x_{t+1}, dx_{t+1} on entry to step t.
    double P0 = 0.0, P1 = 0.0, D0 = 0.0, D1 = 0.0;   // p_{t+1}, dp_{t+1}
    double gA00 = 0.0, gA01 = 0.0, gA10 = 0.0, gA11 = 0.0, gC0 = 0.0, gC1 = 0.0, gQ0 = 0.0, gQ1 = 0.0;
    double gB0[2] = {0.0, 0.0}, gB1[2] = {0.0, 0.0}, gR[2] = {0.0, 0.0}, gLo[2] = {0.0, 0.0}, gHi[2] = {0.0, 0.0};
    double kkt = 0.0;
    for (int t = H - 1; t >= 0; --t) {
        const double tg0 = in(a.targets, 2 * t), tg1 = in(a.targets, 2 * t + 1);
        fin = fin && gfinite(tg0) && gfinite(tg1);
        const double e0 = x0 - tg0, e1 = x1 - tg1;
        const double Qd0 = q0 * d0, Qd1 = q1 * d1;
        if (a.dtargets) {
            a.dtargets[(int64_t)(2 * t) * ld + k] = Qd0;
            a.dtargets[(int64_t)(2 * t + 1) * ld + k] = Qd1;
        }
        gQ0 = gfma(-e0, d0, gQ0);
        gQ1 = gfma(-e1, d1, gQ1);
        // p_t = A' p_{t+1} + Q e_{t+1},  dp_t = A' dp_{t+1} + Q dx_{t+1}
        const double p0 = gfma(a00, P0, gfma(a10, P1, q0 * e0)), p1 = gfma(a01, P0, gfma(a11, P1, q1 * e1));
        const double dp0 = gfma(a00, D0, gfma(a10, D1, Qd0)), dp1 = gfma(a01, D0, gfma(a11, D1, Qd1));
        P0 = p0; P1 = p1; D0 = dp0; D1 = dp1;
        x0 = slot(0, t); x1 = slot(1, t); d0 = slot(2, t); d1 = slot(3, t);
        gC0 = gC0 - dp0;
        gC1 = gC1 - dp1;
        gA00 = gfma(-dp0, x0, gfma(-p0, d0, gA00));
        gA01 = gfma(-dp0, x1, gfma(-p0, d1, gA01));
        gA10 = gfma(-dp1, x0, gfma(-p1, d0, gA10));
        gA11 = gfma(-dp1, x1, gfma(-p1, d1, gA11));
#pragma unroll
        for (int j = 0; j < I; ++j) {
            const double u = in(a.u, t * I + j), g = in(a.g, t * I + j), w = slot(4 + j, t);
            gR[j] = gfma(-w, u, gR[j]);
            gB0[j] = gfma(-dp0, u, gfma(-p0, w, gB0[j]));
            gB1[j] = gfma(-dp1, u, gfma(-p1, w, gB1[j]));
            if (u <= lo[j]) {
                gLo[j] = gLo[j] + (g - gfma(b0[j], dp0, gfma(b1[j], dp1, r[j] * w)));
            } else if (u >= hi[j]) {
                gHi[j] = gHi[j] + (g - gfma(b0[j], dp0, gfma(b1[j], dp1, r[j] * w)));
            } else {
                const double df = gfma(b0[j], p0, gfma(b1[j], p1, r[j] * u));
                kkt = gabs(df) > kkt ? gabs(df) : kkt;
            }
        }
    }

    const uint32_t flags = (fin ? 0u : 0x1u) | (ok ? 0u : 0x4u);
    const bool zero = flags != 0u;
    auto out = [&](double* base, int c, double v) { if (base) base[(int64_t)c * ld + k] = zero ? 0.0 : v; };
    if (zero && a.dtargets)
        for (int t = 0; t < 2 * H; ++t) a.dtargets[(int64_t)t * ld + k] = 0.0;
    out(a.dA, 0, gA00); out(a.dA, 1, gA01); out(a.dA, 2, gA10); out(a.dA, 3, gA11);
    out(a.dC, 0, gC0); out(a.dC, 1, gC1);
    out(a.dQ, 0, gQ0); out(a.dQ, 1, gQ1);
    out(a.dx0, 0, -gfma(a00, D0, a10 * D1));
    out(a.dx0, 1, -gfma(a01, D0, a11 * D1));
    out(a.kkt, 0, kkt);
#pragma unroll
    for (int j = 0; j < I; ++j) {
        out(a.dB, j, gB0[j]); out(a.dB, I + j, gB1[j]);
        out(a.dR, j, gR[j]); out(a.dlo, j, gLo[j]); out(a.dhi, j, gHi[j]);
    }
    return flags;
}

}  // namespace grad
}  // namespace tpc
