// The exact compact solve (tpc_mpc_solve_batch_compact_exact, include/tpc_mpc.h): phase 1 of ONE instance, shared by
// the gfx950 kernels (mpc_newton_compact.hip) and the host path of the same entry.  It runs the polish's rounds,
// polish::newton_rounds<2> (mpc_polish_model.h), on the reference controller's model, started from U = 0:
//   - the model comes from v and the call's parameters, in registers: A = [1, Tv; 0, 1], B = [0, Tv; Tv/l, -Tv/l],
//     C = 0, x0 = 0, every target (dy, dphi) -- no model or target array is read;
//   - the per-step values go through one pointer, ws[(q * H + t) * wn]: the handle's gradient workspace (run-time H),
//     or, with a compile-time horizon HC, an array of the lane's own whose every index is then a constant, so that it
//     lives in registers (a private array indexed by a run-time step lands in scratch).
// The rounds are the general form's own function on the expanded values -- the "+ C" and the x0 terms included:
// fma(a, b, +0) is not a * b when the product is -0 -- so the result equals tpc_mpc_polish_batch_general on the expanded
// arrays with zero controls bit for bit (tests/test_compact_exact_host.py).  What is this header's own: the model, the
// start (cold or WARM), the outputs, and which inputs count as non-finite.
// Every fused operation is an explicit fma() and the unit is built with -ffp-contract=off, as mpc_polish_model.h.
#pragma once

#include "mpc_polish_model.h"

namespace tpc {
namespace cexact {

using grad::gfinite;
using polish::clampd;

// v, dy, dphi [n]; the outputs: front, rear [n], seq [H*2] rows ld_seq apart (may be null), and the optional rows of
// the polish (status, residuals) and fell_back [n], which phase 1 clears
struct Args {
    int64_t n;
    const double *v, *dy, *dphi;
    double T, l, q0, q1, r[2], lo[2], hi[2];   // tpc_mpc_params: step_size, wheelbase, weights, bounds
    const double* params;   // the rows entries: [10] rows ld_params apart, the ten values of instance k in column k, in
    int64_t ld_params;      // cgrad's order (q0 q1 r[0] r[1] T l lo[0] lo[1] hi[0] hi[1]); the ten fields above are unused
    double tol;
    int32_t max_rounds;
    int32_t raise_not_polished;   // FALLBACK_NONE: an unverified instance raises TPC_MPC_FLAG_NOT_POLISHED
    double *front, *rear, *seq;
    int64_t ld_seq;
    int32_t* status;
    double *res_in, *res_out;
    int32_t* fell_back;
    int32_t* fb_index;    // [n] the instances for the fallback, in no particular order; null: not collected
    uint32_t* fb_count;   // how many
    const double* start;  // the warm entry (exact_instance<.., WARM = true>): [H*2] rows ld_start apart, the start of
    int64_t ld_start;     // instance k in column k; may be seq (a lane reads its column before its first write)
};

constexpr int kI = 2;
constexpr int kSlots = polish::slots(kI);   // workspace doubles per step

// The ten model values of instance k.  ROWS: column k of a.params, each loaded once; otherwise the call's own, from the
// kernel arguments.  The return value is a's ten fields either way, so build_model serves both.
template <bool ROWS>
TPC_GRAD_HD Args instance_params(const Args& a, int64_t k) {
    if (!ROWS) return a;
    Args b = a;
    const double* p = a.params + k;
    const int64_t ld = a.ld_params;
    b.q0 = p[0]; b.q1 = p[ld]; b.r[0] = p[2 * ld]; b.r[1] = p[3 * ld];
    b.T = p[4 * ld]; b.l = p[5 * ld];
    b.lo[0] = p[6 * ld]; b.lo[1] = p[7 * ld]; b.hi[0] = p[8 * ld]; b.hi[1] = p[9 * ld];
    return b;
}

// the expanded model of one instance, as mpc_compact (autograd.py) builds it; fin / ok as grad::load_model has them
TPC_GRAD_HD grad::Model build_model(const Args& a, double v) {
    const double Tv = a.T * v, tvl = Tv / a.l;
    grad::Model m;
    m.a00 = 1.0; m.a01 = Tv; m.a10 = 0.0; m.a11 = 1.0;
    m.c0 = 0.0; m.c1 = 0.0; m.q0 = a.q0; m.q1 = a.q1;
    m.b0[0] = 0.0; m.b0[1] = Tv;
    m.b1[0] = tvl; m.b1[1] = -tvl;
    m.fin = gfinite(v) && gfinite(Tv) && gfinite(tvl) && gfinite(m.q0) && gfinite(m.q1);
    m.ok = m.q0 >= 0.0 && m.q1 >= 0.0;
#pragma unroll
    for (int j = 0; j < kI; ++j) {
        m.r[j] = a.r[j]; m.lo[j] = a.lo[j]; m.hi[j] = a.hi[j];
        m.fin = m.fin && gfinite(m.r[j]) && m.lo[j] == m.lo[j] && m.hi[j] == m.hi[j];
        m.ok = m.ok && m.r[j] > 0.0 && m.hi[j] >= m.lo[j];
    }
    return m;
}

// One instance.  HC > 0: the horizon, at compile time (Hrt is ignored); HC == 0: Hrt.  ws points at the instance's
// first workspace element.  Returns its TPC_MPC_FLAG_* bits: 0x1 non-finite, 0x4 bad model (both: nothing run), 0x8
// not verified; in all three cases the outputs are zeros with status -1 (residual_in keeps round 0's value when rounds
// were run, as the polish reports it).
// WARM (tpc_mpc_solve_batch_compact_exact_from): the working copy starts at the clamped column k of a.start where the
// parents start at clampd(0.0, ..); a column with a non-finite component means "no start" and is the parents' start in
// every component.  WARM = false compiles to the parents' code: a.start is not read.
template <int HC, bool ROWS = false, bool WARM = false>
TPC_GRAD_HD uint32_t exact_instance(const Args& a, int Hrt, int64_t k, double* ws, int64_t wn) {
    constexpr int I = kI;
    const int H = HC > 0 ? HC : Hrt;
    auto slot = [&](int q, int t) -> double& { return ws[((int64_t)q * H + t) * wn]; };
    const double tg0 = a.dy[k], tg1 = a.dphi[k];
    const Args pa = instance_params<ROWS>(a, k);
    const grad::Model m = build_model(pa, a.v[k]);
    const double xs0 = 0.0, xs1 = 0.0;
    // the rows entries decide a non-finite T or l per instance (l = inf leaves Tv / l finite); the call's own are checked
    // before the launch
    const bool fin = m.fin && gfinite(tg0) && gfinite(tg1) && (!ROWS || (gfinite(pa.T) && gfinite(pa.l)));
    constexpr int kU = 4 + I;   // first slot of the working copy

    auto finish = [&](int32_t status, double r_in, double r_out) {
        if (a.status) a.status[k] = status;
        if (a.res_in) a.res_in[k] = r_in;
        if (a.res_out) a.res_out[k] = r_out;
        if (a.fell_back) a.fell_back[k] = 0;
        a.front[k] = status >= 0 ? slot(kU, 0) : 0.0;
        a.rear[k] = status >= 0 ? slot(kU + 1, 0) : 0.0;
        if (a.seq)
            for (int t = 0; t < H; ++t)
#pragma unroll
                for (int j = 0; j < I; ++j)
                    a.seq[(int64_t)(t * I + j) * a.ld_seq + k] = status >= 0 ? slot(kU + j, t) : 0.0;
    };
    const uint32_t bad = (fin ? 0u : 0x1u) | (m.ok ? 0u : 0x4u);
    if (bad) {
        finish(-1, 0.0, 0.0);
        return bad;
    }
    if (WARM) {
        // one pass over the column: clamp into the slots and track finiteness of what was loaded (the clamp would hide
        // an Inf); the slots are rewritten only for a column that was not finite
        bool have = true;
        for (int t = 0; t < H; ++t)
#pragma unroll
            for (int j = 0; j < I; ++j) {
                const double s = a.start[(int64_t)(t * I + j) * a.ld_start + k];
                have = have && gfinite(s);
                slot(kU + j, t) = clampd(s, m.lo[j], m.hi[j]);
            }
        if (!have)
            for (int t = 0; t < H; ++t)
#pragma unroll
                for (int j = 0; j < I; ++j) slot(kU + j, t) = clampd(0.0, m.lo[j], m.hi[j]);
    } else {
        for (int t = 0; t < H; ++t)
#pragma unroll
            for (int j = 0; j < I; ++j) slot(kU + j, t) = clampd(0.0, m.lo[j], m.hi[j]);
    }

    double res_in = 0.0, res_out = 0.0;
    const int32_t round = polish::newton_rounds<I>(
        m, H, xs0, xs1, [&](int, int c) { return c == 0 ? tg0 : tg1; }, a.tol, a.max_rounds, ws, wn, res_in, res_out);
    if (round >= 0) {
        finish(round, res_in, res_out);
        return 0u;
    }
    // the one difference from polish_instance's outputs: that leaves the caller's sequence and reports residual_out =
    // residual_in; an unverified instance here has zeros for outputs, and its residual_out is one of them
    finish(-1, res_in, 0.0);
    return 0x8u;
}

}  // namespace cexact
}  // namespace tpc
