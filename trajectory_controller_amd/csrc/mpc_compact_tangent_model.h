// Forward-mode derivative of the exact compact solve (tpc_mpc_solve_batch_compact_exact_forward, include/tpc_mpc.h): the
// arithmetic of ONE (direction, instance) pair, shared by the gfx950 kernels (mpc_compact_tangent.hip) and the host path
// of the same entry.  It is tangent::step<2> (mpc_tangent_model.h), as it is, on the model cexact::build_model
// (mpc_newton_compact_model.h) makes from v in registers -- C = 0, x0 = 0, every target (dy, dphi) -- with the model's
// tangent built in registers by the chain rule of that model building:
//   a01 = b0[1] = Tv, b1[0] = Tv / l, b1[1] = -(Tv / l), Tv = T * v, so
//   tTv = tT v + T tv        ttvl = (tTv - (Tv / l) tl) / l
//   ta01 = tb0[1] = tTv, tb1[0] = ttvl, tb1[1] = -ttvl, every other entry of tA, tB, tC is zero,
//   tx0 = 0, every target's tangent (tdy, tdphi), and tQ, tR and the bounds' tangents pass through.
// No model, target or tangent row of the general form is read or written: 3 + 2H doubles and the direction's values in,
// two doubles (and the optional tangent sequence) out.  The per-step values go through one pointer, ws[(q * H + t) * wn],
// as in mpc_compact_grad_model.h: the handle's gradient workspace, or with a compile-time horizon an array of the lane's
// own.  Every operation of the chain rule is rounded on its own (-ffp-contract=off), so kernels and host path give the
// same bits, and both equal tpc_mpc_solve_batch_general_forward on the expanded arrays and tangents as numbers
// (tests/test_compact_tangent_host.py).  The map is the transpose of cgrad::compact_grad_instance to rounding.
#pragma once

#include "mpc_newton_compact_model.h"
#include "mpc_tangent_model.h"

namespace tpc {
namespace ctan {

using grad::gfinite;

constexpr int kI = 2;
constexpr int kParams = 10;   // cgrad's order: q0 q1 r[0] r[1] T l lo[0] lo[1] hi[0] hi[1]

// v, dy, dphi [n], seq [H*2] rows ld apart, status [n] (may be null); the K directions (any may be null: zero): tv, tdy,
// tdphi [K] rows ld apart, and the parameters' tangent, either tparams [K*10] elements, shared by the instances, or
// tparams_rows [K*10] rows ld apart; the outputs (any may be null): tfront, trear [K], tseq [K*H*2] rows ld apart
struct Args {
    int64_t n, ld;
    int K;
    const double *v, *dy, *dphi, *seq;
    const int32_t* status;
    double T, l, q0, q1, r[2], lo[2], hi[2];   // tpc_mpc_params: step_size, wheelbase, weights, bounds
    const double* params;   // given params_rows: [10] rows ld apart, instance k's own ten values in column k; the ten
                            // fields above are unused
    const double *tv, *tdy, *tdphi, *tparams, *tparams_rows;
    double *tfront, *trear, *tseq;
};

// workspace doubles per step
TPC_GRAD_HD constexpr int slots(bool whole) { return tangent::slots(kI, whole); }

// Direction d of instance k.  HC > 0: the horizon, at compile time (Hrt is ignored); HC == 0: Hrt.  ws points at the
// lane's first workspace element.  WHOLE: a.tseq receives the whole tangent sequence.  Returns the TPC_MPC_FLAG_* bits
// (0x1 non-finite, 0x4 bad model); a flagged (d, k) pair has zeros for outputs, and so has an instance with a negative
// status, without a flag of its own.
// ROWS: the model, T and l are instance k's own (a.params), and the parameters' tangent is a.tparams_rows.
template <int HC, bool ROWS, bool WHOLE>
TPC_GRAD_HD uint32_t compact_tangent_instance(const Args& a, int Hrt, int d, int64_t k, double* ws, int64_t wn) {
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

    // the direction's values
    auto dir = [&](const double* base) -> double { return base ? base[(int64_t)d * ld + k] : 0.0; };
    const double tv = dir(a.tv), ttg0 = dir(a.tdy), ttg1 = dir(a.tdphi);
    double tp[kParams];
#pragma unroll
    for (int c = 0; c < kParams; ++c) {
        if (ROWS) tp[c] = a.tparams_rows ? a.tparams_rows[((int64_t)d * kParams + c) * ld + k] : 0.0;
        else tp[c] = a.tparams ? a.tparams[d * kParams + c] : 0.0;
    }

    // the chain rule of build_model
    const double tT = tp[4], tl = tp[5];
    const double tvl = m.b1[0];   // Tv / l
    const double tTv = tT * v + T * tv;
    const double ttvl = (tTv - tvl * tl) / l;
    grad::Model tm;
    tm.a00 = 0.0; tm.a01 = tTv; tm.a10 = 0.0; tm.a11 = 0.0;
    tm.c0 = 0.0; tm.c1 = 0.0; tm.q0 = tp[0]; tm.q1 = tp[1];
    tm.b0[0] = 0.0; tm.b0[1] = tTv;
    tm.b1[0] = ttvl; tm.b1[1] = -ttvl;
    tm.fin = gfinite(tv) && gfinite(tT) && gfinite(tl) && gfinite(tTv) && gfinite(ttvl) && gfinite(tm.q0) &&
             gfinite(tm.q1);
    tm.ok = true;
#pragma unroll
    for (int j = 0; j < I; ++j) {
        tm.r[j] = tp[2 + j]; tm.lo[j] = tp[6 + j]; tm.hi[j] = tp[8 + j];
        tm.fin = tm.fin && gfinite(tm.r[j]) && gfinite(tm.lo[j]) && gfinite(tm.hi[j]);
    }

    double* ts = WHOLE ? a.tseq + ((int64_t)d * H * I) * ld + k : nullptr;
    double tu0[2];
    const bool fin = tangent::step<I, WHOLE>(
                         m, tm, H, 0.0, 0.0, 0.0, 0.0, [&](int t, int j) { return a.seq[(int64_t)(t * I + j) * ld + k]; },
                         [&](int, int c) { return c == 0 ? tg0 : tg1; }, [&](int, int c) { return c == 0 ? ttg0 : ttg1; },
                         [&](int t, int j, double x) { ts[(int64_t)(t * I + j) * ld] = x; }, ws, wn, tu0) &&
                     m.fin && tm.fin && (!ROWS || (gfinite(T) && gfinite(l)));   // as cexact::exact_instance decides it

    const uint32_t flags = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    const bool zero = flags != 0u || (a.status && a.status[k] < 0);
    const int64_t o = (int64_t)d * ld + k;
    if (a.tfront) a.tfront[o] = zero ? 0.0 : tu0[0];
    if (a.trear) a.trear[o] = zero ? 0.0 : tu0[1];
    if (WHOLE && zero)
        for (int c = 0; c < H * I; ++c) ts[(int64_t)c * ld] = 0.0;
    return flags;
}

}  // namespace ctan
}  // namespace tpc
