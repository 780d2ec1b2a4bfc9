// Backward passes of the general form (tpc_mpc_solve_batch_general_backward and tpc_mpc_rollout_backward,
// include/tpc_mpc.h): the arithmetic of ONE instance, shared by the gfx950 kernels (mpc_grad.hip, mpc_rollout_grad.hip)
// and the host paths of the same entries.  Every fused operation is an explicit fma() and the translation units are built
// with -ffp-contract=off, so the kernels and the host paths give the same bits (tests/test_grad_gpu.py,
// tests/test_rollout_grad_gpu.py hold them to it).
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
// qp_step() is that derivative for one solve, on accessors for u, g and the targets; it accumulates into a Sums and
// hands each dL/dtarget_t to a callback.  instance() is the single solve; rollout_instance() chains qp_step over the
// steps of a closed loop in reverse (the sweep of include/tpc_mpc.h, tpc_mpc_rollout_backward).
//
// Three passes over the horizon, no per-step array in registers or private memory (a private array indexed by the step
// lands in scratch): the per-step quantities live in a workspace of slots(I) doubles per step, element (q, t) of
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

// ... and of the closed loop: the io's model and initial state / targets, the rollout's new_last_targets [steps*2],
// recorded sequences [steps*H*I] and states [steps*2], dL/dcontrols_out [steps*I], dL/dstates_out [steps*2] (either
// may be null: zero), and the outputs, dnlt [steps*2] among them
struct RollArgs {
    int64_t n, ld;
    int steps;
    const double *A, *B, *C, *Q, *R, *lo, *hi, *x0, *targets, *nlt, *seq, *states, *gu, *gx;
    double *dA, *dB, *dC, *dQ, *dR, *dlo, *dhi, *dx0, *dtargets, *dnlt, *kkt;
};

// The separate plant of tpc_mpc_rollout_plant_backward: x_{k+1} = Ap x_k + Bp u0_k + Cp (+ d_k).  A, B, C are never
// null here: the caller passes the controller's arrays again when it gave no plant, with separate = 0, and the plant
// terms then go into the controller's dA, dB, dC as in rollout_instance<I, false>.  With separate = 1 they go to dA,
// dB, dC below (any may be null) and the controller's receive qp_step's contributions only.  dd [steps*2] (leading
// dimension ld_d, may be null) receives mu_k = dL/dx_{k+1}, the gradient of the disturbance's row k.
struct RollPlant {
    const double *A, *B, *C;
    double *dA, *dB, *dC, *dd;
    int64_t ld_d;
    int separate;
};

// the plant's own gradient sums (RollPlant::separate): the fields of Sums the plant line adds to
struct PlantSums {
    double A00 = 0.0, A01 = 0.0, A10 = 0.0, A11 = 0.0, C0 = 0.0, C1 = 0.0;
    double B0[2] = {0.0, 0.0}, B1[2] = {0.0, 0.0};
};

// workspace doubles per step: gain + feed-forward (3 I) in pass 1, x, dx, w (4 + I) from pass 2 on
TPC_GRAD_HD constexpr int slots(int I) { return 4 + I; }

TPC_GRAD_HD double gfma(double a, double b, double c) { return __builtin_fma(a, b, c); }
TPC_GRAD_HD double gabs(double x) { return __builtin_fabs(x); }
TPC_GRAD_HD bool gfinite(double x) { return gabs(x) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// one instance's model (B, R and the bounds per input; constant indices only), with its finiteness and dlib's
// requires clause (min(Q) >= 0, min(R) > 0, upper >= lower)
struct Model {
    double a00, a01, a10, a11, c0, c1, q0, q1;
    double b0[2], b1[2], r[2], lo[2], hi[2];   // row 0 / row 1 of B, per input
    bool fin, ok;
};

template <int I>
TPC_GRAD_HD Model load_model(const double* A, const double* B, const double* C, const double* Q, const double* R,
                             const double* lo, const double* hi, int64_t ld, int64_t k) {
    auto in = [&](const double* base, int c) -> double { return base[(int64_t)c * ld + k]; };
    Model m;
    m.a00 = in(A, 0); m.a01 = in(A, 1); m.a10 = in(A, 2); m.a11 = in(A, 3);
    m.c0 = in(C, 0); m.c1 = in(C, 1); m.q0 = in(Q, 0); m.q1 = in(Q, 1);
    m.fin = gfinite(m.a00) && gfinite(m.a01) && gfinite(m.a10) && gfinite(m.a11) && gfinite(m.c0) && gfinite(m.c1) &&
            gfinite(m.q0) && gfinite(m.q1);
    m.ok = m.q0 >= 0.0 && m.q1 >= 0.0;
#pragma unroll
    for (int j = 0; j < I; ++j) {
        m.b0[j] = in(B, j);
        m.b1[j] = in(B, I + j);
        m.r[j] = in(R, j);
        m.lo[j] = in(lo, j);
        m.hi[j] = in(hi, j);
        m.fin = m.fin && gfinite(m.b0[j]) && gfinite(m.b1[j]) && gfinite(m.r[j]) && m.lo[j] == m.lo[j] &&
                m.hi[j] == m.hi[j];
        m.ok = m.ok && m.r[j] > 0.0 && m.hi[j] >= m.lo[j];
    }
    return m;
}

// gradient sums of the model's inputs (accumulated over the steps of a closed loop) and the residual
struct Sums {
    double A00 = 0.0, A01 = 0.0, A10 = 0.0, A11 = 0.0, C0 = 0.0, C1 = 0.0, Q0 = 0.0, Q1 = 0.0;
    double B0[2] = {0.0, 0.0}, B1[2] = {0.0, 0.0}, R[2] = {0.0, 0.0}, lo[2] = {0.0, 0.0}, hi[2] = {0.0, 0.0};
    double kkt = 0.0;
};

// Passes 1 and 2 of the header comment for one QP: w = H_FF^-1 g_F (w = 0 off F) by the masked Riccati sweep, F given
// by free_at(j, u, g) on the values u(t, j), g(t, j) that u_at and g_at read.  Pass 1 reads step t's u and g before it
// writes step t's slots, so g may live in the feed-forward's slot (2 I + j, t).  Leaves x_t, dx_t, w_t in the step's slots
// and x_H, dx_H in (x0, x1, d0, d1); clears fin if a u or g read is not finite.  Shared by qp_step() and by
// polish::newton_rounds() (mpc_polish_model.h).
template <int I, class U, class G, class FR>
TPC_GRAD_HD void riccati_passes(const Model& m, int H, double xs0, double xs1, U u_at, G g_at, FR free_at, double* ws,
                                int64_t wn, bool& fin, double& x0, double& x1, double& d0, double& d1) {
    auto slot = [&](int q, int t) -> double& { return ws[((int64_t)q * H + t) * wn]; };
    const double a00 = m.a00, a01 = m.a01, a10 = m.a10, a11 = m.a11, c0 = m.c0, c1 = m.c1, q0 = m.q0, q1 = m.q1;

    // ---- 1. masked Riccati sweep, t = H-1 .. 0.  V_{t+1}(dx) = 1/2 dx' P dx + s' dx, P = s = 0 at t + 1 = H.
    double p00 = 0.0, p01 = 0.0, p11 = 0.0, s0 = 0.0, s1 = 0.0;
    for (int t = H - 1; t >= 0; --t) {
        double u[2], g[2];
        bool fr[2];
#pragma unroll
        for (int j = 0; j < I; ++j) {
            u[j] = u_at(t, j);
            g[j] = g_at(t, j);
            fin = fin && gfinite(u[j]) && gfinite(g[j]);
            fr[j] = free_at(j, u[j], g[j]);
        }
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
        double K0[2], K1[2], kf[2];
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
            slot(2 * j, t) = K0[j];
            slot(2 * j + 1, t) = K1[j];
            slot(2 * I + j, t) = kf[j];
        }
        p00 = n00; p01 = n01; p11 = n11; s0 = m0; s1 = m1;
    }

    // ---- 2. forward: x_t, dx_t, w_t -> the step's slots (0, 1: x; 2, 3: dx; 4..: w)
    x0 = xs0; x1 = xs1; d0 = 0.0; d1 = 0.0;
    for (int t = 0; t < H; ++t) {
        double w[2], u[2];
#pragma unroll
        for (int j = 0; j < I; ++j) {
            w[j] = gfma(slot(2 * j, t), d0, gfma(slot(2 * j + 1, t), d1, slot(2 * I + j, t)));
            u[j] = u_at(t, j);
        }
        slot(0, t) = x0; slot(1, t) = x1; slot(2, t) = d0; slot(3, t) = d1;
#pragma unroll
        for (int j = 0; j < I; ++j) slot(4 + j, t) = w[j];
        double y0 = gfma(a00, x0, gfma(a01, x1, c0)), y1 = gfma(a10, x0, gfma(a11, x1, c1));
        double e0 = gfma(a00, d0, a01 * d1), e1 = gfma(a10, d0, a11 * d1);
#pragma unroll
        for (int j = 0; j < I; ++j) {
            y0 = gfma(m.b0[j], u[j], y0);
            y1 = gfma(m.b1[j], u[j], y1);
            e0 = gfma(m.b0[j], w[j], e0);
            e1 = gfma(m.b1[j], w[j], e1);
        }
        x0 = y0; x1 = y1; d0 = e0; d1 = e1;
    }
}

// The derivative of one solve from state (xs0, xs1): u(t, j), g(t, j) and tg(t, c) read the controls, dL/du and the
// targets; dtg(t, v0, v1) receives dL/dtarget_t.  Adds the gradients to s, raises s.kkt to the step's residual, and
// returns dL/dx0 in (dx00, dx01).  Returns false if a control, a dL/du or a target read is not finite.
template <int I, class U, class G, class TG, class DTG>
TPC_GRAD_HD bool qp_step(const Model& m, int H, double xs0, double xs1, U u_at, G g_at, TG tg_at, DTG dtg, double* ws,
                         int64_t wn, Sums& s, double& dx00, double& dx01) {
    auto slot = [&](int q, int t) -> double& { return ws[((int64_t)q * H + t) * wn]; };
    const double a00 = m.a00, a01 = m.a01, a10 = m.a10, a11 = m.a11, q0 = m.q0, q1 = m.q1;
    bool fin = true;

    // ---- 1, 2. the Riccati sweep and the forward pass, F = the components strictly inside the box
    double x0, x1, d0, d1;
    riccati_passes<I>(
        m, H, xs0, xs1, u_at, g_at, [&](int j, double u, double) { return !(u <= m.lo[j] || u >= m.hi[j]); }, ws, wn,
        fin, x0, x1, d0, d1);

    // ---- 3. backward: costates and gradients.  (x0, x1, d0, d1) hold x_{t+1}, dx_{t+1} on entry to step t.
    double P0 = 0.0, P1 = 0.0, D0 = 0.0, D1 = 0.0;   // p_{t+1}, dp_{t+1}
    for (int t = H - 1; t >= 0; --t) {
        const double tg0 = tg_at(t, 0), tg1 = tg_at(t, 1);
        fin = fin && gfinite(tg0) && gfinite(tg1);
        const double e0 = x0 - tg0, e1 = x1 - tg1;
        const double Qd0 = q0 * d0, Qd1 = q1 * d1;
        dtg(t, Qd0, Qd1);
        s.Q0 = gfma(-e0, d0, s.Q0);
        s.Q1 = gfma(-e1, d1, s.Q1);
        // p_t = A' p_{t+1} + Q e_{t+1},  dp_t = A' dp_{t+1} + Q dx_{t+1}
        const double p0 = gfma(a00, P0, gfma(a10, P1, q0 * e0)), p1 = gfma(a01, P0, gfma(a11, P1, q1 * e1));
        const double dp0 = gfma(a00, D0, gfma(a10, D1, Qd0)), dp1 = gfma(a01, D0, gfma(a11, D1, Qd1));
        P0 = p0; P1 = p1; D0 = dp0; D1 = dp1;
        x0 = slot(0, t); x1 = slot(1, t); d0 = slot(2, t); d1 = slot(3, t);
        s.C0 = s.C0 - dp0;
        s.C1 = s.C1 - dp1;
        s.A00 = gfma(-dp0, x0, gfma(-p0, d0, s.A00));
        s.A01 = gfma(-dp0, x1, gfma(-p0, d1, s.A01));
        s.A10 = gfma(-dp1, x0, gfma(-p1, d0, s.A10));
        s.A11 = gfma(-dp1, x1, gfma(-p1, d1, s.A11));
#pragma unroll
        for (int j = 0; j < I; ++j) {
            const double u = u_at(t, j), g = g_at(t, j), w = slot(4 + j, t);
            s.R[j] = gfma(-w, u, s.R[j]);
            s.B0[j] = gfma(-dp0, u, gfma(-p0, w, s.B0[j]));
            s.B1[j] = gfma(-dp1, u, gfma(-p1, w, s.B1[j]));
            if (u <= m.lo[j]) {
                s.lo[j] = s.lo[j] + (g - gfma(m.b0[j], dp0, gfma(m.b1[j], dp1, m.r[j] * w)));
            } else if (u >= m.hi[j]) {
                s.hi[j] = s.hi[j] + (g - gfma(m.b0[j], dp0, gfma(m.b1[j], dp1, m.r[j] * w)));
            } else {
                const double df = gfma(m.b0[j], p0, gfma(m.b1[j], p1, m.r[j] * u));
                s.kkt = gabs(df) > s.kkt ? gabs(df) : s.kkt;
            }
        }
    }
    dx00 = -gfma(a00, D0, a10 * D1);
    dx01 = -gfma(a01, D0, a11 * D1);
    return fin;
}

// the model's gradient outputs of one instance (zeros when flagged)
template <int I>
TPC_GRAD_HD void store_sums(const Sums& s, bool zero, int64_t ld, int64_t k, double* dA, double* dB, double* dC,
                            double* dQ, double* dR, double* dlo, double* dhi, double* kkt) {
    auto out = [&](double* base, int c, double v) { if (base) base[(int64_t)c * ld + k] = zero ? 0.0 : v; };
    out(dA, 0, s.A00); out(dA, 1, s.A01); out(dA, 2, s.A10); out(dA, 3, s.A11);
    out(dC, 0, s.C0); out(dC, 1, s.C1);
    out(dQ, 0, s.Q0); out(dQ, 1, s.Q1);
    out(kkt, 0, s.kkt);
#pragma unroll
    for (int j = 0; j < I; ++j) {
        out(dB, j, s.B0[j]); out(dB, I + j, s.B1[j]);
        out(dR, j, s.R[j]); out(dlo, j, s.lo[j]); out(dhi, j, s.hi[j]);
    }
}

// One instance of the single solve.  ws points at the instance's first workspace element (ws[(q * H + t) * wn]).
// Returns its TPC_MPC_FLAG_* bits (0x1 non-finite, 0x4 bad model); a flagged instance gets all-zero outputs.
template <int I>
TPC_GRAD_HD uint32_t instance(const Args& a, int H, int64_t k, double* ws, int64_t wn) {
    const int64_t ld = a.ld;
    auto in = [&](const double* base, int c) -> double { return base[(int64_t)c * ld + k]; };
    const Model m = load_model<I>(a.A, a.B, a.C, a.Q, a.R, a.lo, a.hi, ld, k);
    const double xs0 = in(a.x0, 0), xs1 = in(a.x0, 1);
    bool fin = m.fin && gfinite(xs0) && gfinite(xs1);
    Sums s;
    double dx00, dx01;
    fin = qp_step<I>(
              m, H, xs0, xs1, [&](int t, int j) { return in(a.u, t * I + j); },
              [&](int t, int j) { return in(a.g, t * I + j); }, [&](int t, int c) { return in(a.targets, 2 * t + c); },
              [&](int t, double v0, double v1) {
                  if (a.dtargets) {
                      a.dtargets[(int64_t)(2 * t) * ld + k] = v0;
                      a.dtargets[(int64_t)(2 * t + 1) * ld + k] = v1;
                  }
              },
              ws, wn, s, dx00, dx01) && fin;

    const uint32_t flags = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    const bool zero = flags != 0u;
    if (zero && a.dtargets)
        for (int t = 0; t < 2 * H; ++t) a.dtargets[(int64_t)t * ld + k] = 0.0;
    store_sums<I>(s, zero, ld, k, a.dA, a.dB, a.dC, a.dQ, a.dR, a.dlo, a.dhi, a.kkt);
    if (a.dx0) {
        a.dx0[k] = zero ? 0.0 : dx00;
        a.dx0[ld + k] = zero ? 0.0 : dx01;
    }
    return flags;
}

// One instance of the closed loop: the reverse sweep over the steps (include/tpc_mpc.h, tpc_mpc_rollout_backward).
// Step k solved from x_k (x0, then the recorded states[k-1]) with the targets T_k of the rollout's shift:
//   T_k[t] = targets[t+k] for t + k <= H-1, else nlt[t+k-(H-1)] (targets[H-1] without nlt).
// dL/dT_k is added into dtargets / dnlt through the same map, so both are zeroed first.  lambda = dL/dx_k carries the
// state gradient from step to step in registers; the workspace is reused by every step.
// With Plant (tpc_mpc_rollout_plant_backward) the state moves with pl's arrays: they are read at the step, where the
// update's terms are formed, and not held across the horizon passes.
template <int I, bool Plant = false>
TPC_GRAD_HD uint32_t rollout_instance(const RollArgs& a, int H, int64_t k, double* ws, int64_t wn,
                                      const RollPlant* pl = nullptr) {
    const int64_t ld = a.ld;
    const int S = a.steps;
    const int HI = H * I;
    auto in = [&](const double* base, int64_t c) -> double { return base[c * ld + k]; };
    auto at = [&](double* base, int64_t c) -> double& { return base[c * ld + k]; };
    const Model m = load_model<I>(a.A, a.B, a.C, a.Q, a.R, a.lo, a.hi, ld, k);
    bool fin = m.fin && gfinite(in(a.x0, 0)) && gfinite(in(a.x0, 1)) && gfinite(in(a.states, 2 * (int64_t)S - 2)) &&
               gfinite(in(a.states, 2 * (int64_t)S - 1));
    if (a.dtargets)
        for (int c = 0; c < 2 * H; ++c) at(a.dtargets, c) = 0.0;
    if (a.dnlt)
        for (int64_t c = 0; c < 2 * (int64_t)S; ++c) at(a.dnlt, c) = 0.0;

    Sums s;
    PlantSums ps;   // the plant's own sums (Plant with pl->separate; unused otherwise)
    double l0 = 0.0, l1 = 0.0;   // lambda = dL/dx_{k+1} from the steps after k
    for (int kk = S - 1; kk >= 0; --kk) {
        const double gx0 = a.gx ? in(a.gx, 2 * (int64_t)kk) : 0.0, gx1 = a.gx ? in(a.gx, 2 * (int64_t)kk + 1) : 0.0;
        const double mu0 = l0 + gx0, mu1 = l1 + gx1;   // total dL/dx_{k+1}
        const double xs0 = kk == 0 ? in(a.x0, 0) : in(a.states, 2 * (int64_t)kk - 2);
        const double xs1 = kk == 0 ? in(a.x0, 1) : in(a.states, 2 * (int64_t)kk - 1);
        fin = fin && gfinite(gx0) && gfinite(gx1) && gfinite(xs0) && gfinite(xs1);
        const int64_t sq = (int64_t)kk * HI;   // first row of U_k
        // the plant update x_{k+1} = A x_k + B u0_k + C: its terms go into t
        double g0[2];   // dL/du0_k = G_u[k] + B' mu
        auto plant_terms = [&](auto& t) {
            t.A00 = gfma(mu0, xs0, t.A00);
            t.A01 = gfma(mu0, xs1, t.A01);
            t.A10 = gfma(mu1, xs0, t.A10);
            t.A11 = gfma(mu1, xs1, t.A11);
            t.C0 = t.C0 + mu0;
            t.C1 = t.C1 + mu1;
#pragma unroll
            for (int j = 0; j < I; ++j) {
                const double u0 = in(a.seq, sq + j);
                const double gu = a.gu ? in(a.gu, (int64_t)kk * I + j) : 0.0;
                fin = fin && gfinite(gu);
                t.B0[j] = gfma(mu0, u0, t.B0[j]);
                t.B1[j] = gfma(mu1, u0, t.B1[j]);
                double b0 = m.b0[j], b1 = m.b1[j];
                if (Plant) {
                    b0 = in(pl->B, j); b1 = in(pl->B, I + j);
                    fin = fin && gfinite(b0) && gfinite(b1);
                }
                g0[j] = gfma(b0, mu0, gfma(b1, mu1, gu));
            }
        };
        if (Plant && pl->separate) plant_terms(ps);
        else plant_terms(s);
        if (Plant && pl->dd) {
            pl->dd[(2 * (int64_t)kk) * pl->ld_d + k] = mu0;
            pl->dd[(2 * (int64_t)kk + 1) * pl->ld_d + k] = mu1;
        }
        // the target map of step kk: component c of T_kk[t] as (base array, component index)
        auto tmap = [&](int t, int c, const double** base) -> int64_t {
            const int r = t + kk;
            if (r <= H - 1) { *base = a.targets; return 2 * r + c; }
            if (a.nlt) { *base = a.nlt; return 2 * (int64_t)(r - (H - 1)) + c; }
            *base = a.targets;
            return 2 * (H - 1) + c;
        };
        double dx00, dx01;
        fin = qp_step<I>(
                  m, H, xs0, xs1, [&](int t, int j) { return in(a.seq, sq + t * I + j); },
                  [&](int t, int j) { return t == 0 ? g0[j] : 0.0; },
                  [&](int t, int c) {
                      const double* b;
                      const int64_t i = tmap(t, c, &b);
                      return in(b, i);
                  },
                  [&](int t, double v0, double v1) {
                      const double* b;
                      const int64_t i = tmap(t, 0, &b);
                      double* d = b == a.targets ? a.dtargets : a.dnlt;
                      if (d) {
                          at(d, i) = at(d, i) + v0;
                          at(d, i + 1) = at(d, i + 1) + v1;
                      }
                  },
                  ws, wn, s, dx00, dx01) && fin;
        // lambda_k = A' mu + dL/dx_k of the solve
        if (Plant) {
            const double a00 = in(pl->A, 0), a01 = in(pl->A, 1), a10 = in(pl->A, 2), a11 = in(pl->A, 3);
            fin = fin && gfinite(a00) && gfinite(a01) && gfinite(a10) && gfinite(a11) && gfinite(in(pl->C, 0)) &&
                  gfinite(in(pl->C, 1));
            l0 = gfma(a00, mu0, gfma(a10, mu1, dx00));
            l1 = gfma(a01, mu0, gfma(a11, mu1, dx01));
        } else {
            l0 = gfma(m.a00, mu0, gfma(m.a10, mu1, dx00));
            l1 = gfma(m.a01, mu0, gfma(m.a11, mu1, dx01));
        }
    }

    const uint32_t flags = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    const bool zero = flags != 0u;
    if (zero && a.dtargets)
        for (int c = 0; c < 2 * H; ++c) at(a.dtargets, c) = 0.0;
    if (zero && a.dnlt)
        for (int64_t c = 0; c < 2 * (int64_t)S; ++c) at(a.dnlt, c) = 0.0;
    store_sums<I>(s, zero, ld, k, a.dA, a.dB, a.dC, a.dQ, a.dR, a.dlo, a.dhi, a.kkt);
    if (Plant) {
        if (pl->separate) {
            auto out = [&](double* base, int c, double v) { if (base) base[(int64_t)c * ld + k] = zero ? 0.0 : v; };
            out(pl->dA, 0, ps.A00); out(pl->dA, 1, ps.A01); out(pl->dA, 2, ps.A10); out(pl->dA, 3, ps.A11);
            out(pl->dC, 0, ps.C0); out(pl->dC, 1, ps.C1);
#pragma unroll
            for (int j = 0; j < I; ++j) { out(pl->dB, j, ps.B0[j]); out(pl->dB, I + j, ps.B1[j]); }
        }
        if (zero && pl->dd)
            for (int64_t c = 0; c < 2 * (int64_t)S; ++c) pl->dd[c * pl->ld_d + k] = 0.0;
    }
    if (a.dx0) {
        at(a.dx0, 0) = zero ? 0.0 : l0;
        at(a.dx0, 1) = zero ? 0.0 : l1;
    }
    return flags;
}

}  // namespace grad
}  // namespace tpc
