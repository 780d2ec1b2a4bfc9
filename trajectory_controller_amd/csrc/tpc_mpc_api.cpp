// C ABI of libtpc_mpc.so (include/tpc_mpc.h): argument validation, host<->device staging, kernel
// family selection.  No solver arithmetic lives here and there is no CPU solve path: every entry
// point ends in a gfx950 kernel launch or fails.  (Mixed-horizon batches: tpc_mpc_mixed.hip; sharded
// solves over RCCL: tpc_mpc_comm.cpp; the resident single-solve kernel: tpc_mpc_one.hip; the gradient kernel and its
// host path for a host-only handle: mpc_grad.hip.)
#include "tpc_mpc_context.h"
#include "tpc_mpc_stage.h"
#include "tpc_mpc_experimental.h"
#include "auto_table.h"
#include "mpc_queue_key_table.h"
#include "mpc_grad_model.h"
#include "mpc_polish_model.h"
#include "mpc_rollout_newton.h"
#include "mpc_newton_compact.h"
#include "mpc_compact_loop.h"
#include "mpc_compact_grad.h"
#include "mpc_compact_loop_grad.h"
#include "mpc_compact_tangent.h"
#include "mpc_tangent_model.h"

#include <cmath>
#include <cstdlib>
#include <mutex>
#include <vector>

namespace tpc {
// per-horizon launchers, one translation unit each (mpc_lane_inst.hip / mpc_wave_inst.hip)
#define TPC_DECL_H(h)                                                                             \
    hipError_t lane_compact_h##h(int, const CompactArgs&, const Knobs&, const Workspace&, hipStream_t); \
    hipError_t lane_general_h##h(int, int, const GeneralArgs&, const Knobs&, const Workspace&, hipStream_t); \
    hipError_t lane_resolve_compact_h##h(const CompactArgs&, const Knobs&, const Workspace&, const int32_t*, const uint32_t*, hipStream_t, double, const uint32_t*, uint32_t); \
    hipError_t lane_presolve_compact_h##h(const CompactArgs&, const Knobs&, const Workspace&, double, uint32_t, hipStream_t); \
    hipError_t lane_resolve_general_h##h(int, const GeneralArgs&, const Knobs&, const Workspace&, const int32_t*, const uint32_t*, hipStream_t, double, const uint32_t*, uint32_t); \
    hipError_t lane_presolve_general_h##h(int, const GeneralArgs&, const Knobs&, const Workspace&, double, uint32_t, hipStream_t); \
    hipError_t wave_compact_h##h(int, const CompactArgs&, const Knobs&, const Workspace&, hipStream_t); \
    hipError_t wave_general_h##h(int, int, const GeneralArgs&, const Knobs&, const Workspace&, hipStream_t); \
    hipError_t ub_compact_h##h(int, int, const CompactArgs&, const Knobs&, const Workspace&, hipStream_t); \
    int64_t lane_rec_len_h##h(int dtype);                                                          \
    const char* lane_build_h##h();
TPC_DECL_H(4) TPC_DECL_H(5) TPC_DECL_H(10) TPC_DECL_H(20) TPC_DECL_H(30) TPC_DECL_H(40)
#undef TPC_DECL_H
// ... and for the general model (mpc_groupg_inst.hip)
#define TPC_DECL_H(h) hipError_t groupg_general_h##h(int, int, int, const GeneralArgs&, const Knobs&, const Workspace&, hipStream_t);
TPC_DECL_H(10) TPC_DECL_H(20) TPC_DECL_H(30) TPC_DECL_H(40)
#undef TPC_DECL_H
// LANE_FMA for the general model (mpc_ubg_inst.hip): N <= 20
#define TPC_DECL_H(h) hipError_t ub_general_h##h(int, int, const GeneralArgs&, const Knobs&, const Workspace&, hipStream_t);
TPC_DECL_H(4) TPC_DECL_H(5) TPC_DECL_H(10) TPC_DECL_H(20)
#undef TPC_DECL_H
// GROUP: G lanes per instance (mpc_group_inst.hip), compact form, the horizons a power of two divides into chunks
#define TPC_DECL_H(h) hipError_t group_compact_h##h(int, int, int, const CompactArgs&, const Knobs&, const Workspace&, hipStream_t);
TPC_DECL_H(10) TPC_DECL_H(20) TPC_DECL_H(30) TPC_DECL_H(40)
#undef TPC_DECL_H

// the backward pass of the general form (mpc_grad.hip)
int64_t grad_scratch_bytes(int I, int H, int64_t n);
hipError_t grad_general(int I, int H, const grad::Args& a, void* ws, uint32_t* flags, hipStream_t s);
uint32_t grad_general_host(int I, int H, const grad::Args& a);
// ... and of the closed loop (mpc_rollout_grad.hip), on the same per-step workspace
hipError_t rollout_grad(int I, int H, const grad::RollArgs& a, void* ws, uint32_t* flags, hipStream_t s);
uint32_t rollout_grad_host(int I, int H, const grad::RollArgs& a);
hipError_t rollout_plant_grad(int I, int H, const grad::RollArgs& a, const grad::RollPlant& pl, void* ws, uint32_t* flags,
                              hipStream_t s);
uint32_t rollout_plant_grad_host(int I, int H, const grad::RollArgs& a, const grad::RollPlant& pl);
// the polish of the general form (mpc_polish.hip), on the gradient workspace grown by the working copy of u
int64_t polish_scratch_bytes(int I, int H, int64_t n);
hipError_t polish_general(int I, int H, const polish::Args& a, void* ws, uint32_t* flags, hipStream_t s);
uint32_t polish_general_host(int I, int H, const polish::Args& a);
// ... and fused with the rollout's step tail (mpc_rollout_polish.hip): one step of tpc_mpc_rollout_polished
hipError_t launch_rollout_polish_step(int I, const polish::Args& p, const RolloutStepArgs& r, void* ws, uint32_t* flags,
                                      hipStream_t s);

// the forward-mode derivatives (mpc_tangent.hip, mpc_rollout_tangent.hip): one lane per (direction, instance), the
// per-step workspace of K * n lanes inside the gradient workspace
int64_t tangent_scratch_bytes(int I, int H, int64_t n, int K, bool whole);
hipError_t tangent_general(int I, int H, const tangent::Args& a, void* ws, uint32_t* flags, hipStream_t s);
uint32_t tangent_general_host(int I, int H, const tangent::Args& a);
hipError_t rollout_tangent(int I, int H, const tangent::RollArgs& a, void* ws, uint32_t* flags, hipStream_t s);
uint32_t rollout_tangent_host(int I, int H, const tangent::RollArgs& a);
hipError_t rollout_plant_tangent(int I, int H, const tangent::RollArgs& a, const tangent::RollPlant& pl, void* ws,
                                 uint32_t* flags, hipStream_t s);
uint32_t rollout_plant_tangent_host(int I, int H, const tangent::RollArgs& a, const tangent::RollPlant& pl);

thread_local char g_create_error[kTpcErrLen] = "";
}  // namespace tpc

using namespace tpc;

static const int kHorizons[] = {4, 5, 10, 20, 30, 40};

namespace {

// horizons with specialised kernels; every other 1 <= H <= kMaxHorizon takes the generic kernel
bool horizon_specialised(int H) {
    for (int h : kHorizons) if (h == H) return true;
    return false;
}
bool horizon_ok(int H) { return H >= 1 && H <= kMaxHorizon; }

Knobs knobs_of(const tpc_mpc_params* p) {
    Knobs k;
    k.eps = p->eps;
    k.max_iter = (uint32_t)p->max_iter;
    k.smo_iters = (uint32_t)p->smo_iters;
    return k;
}

// One-shot: the hint set for this handle applies to the next batch solve of the same size only.
const int32_t* take_hint(tpc_mpc_context* h, int64_t n) {
    const int32_t* p = (h->hint && h->hint_n == n) ? h->hint : nullptr;
    h->hint = nullptr;
    h->hint_n = 0;
    return p;
}

// the host path's translation unit is built with -mfma: only on a CPU that has the instruction
bool host_path_usable() {
#if defined(__x86_64__)
    static const bool ok = __builtin_cpu_supports("fma");
    return ok;
#else
    return true;   // (aarch64: fused multiply-add is baseline)
#endif
}

// Lanes per instance of the GROUP family for horizon H: what TPC_MPC_OPT_GROUP_LANES pins if it divides H, else the
// measured best; 0 where the family has no kernel (N = 4, 5 and the non-specialised horizons).
int group_lanes(const tpc_mpc_context* h, int H, int dtype = 0, int64_t n = 0, int form = 0) {
    if (H != 10 && H != 20 && H != 30 && H != 40) return 0;
    // (what mpc_group_inst.hip / mpc_groupg_inst.hip build: chunks of 3 .. 20 steps -- 3 .. 10 for the general model --
    // padded where G does not divide H)
    auto built = [&](int G) {
        if (H == 10) return G == 2 || G == 4;
        if (form == 1 && H >= 30) return G == 4 || G == 8;
        return G == 2 || G == 4 || G == 8;
    };
    if (form == 1) dtype = TPC_MPC_F64;   // (the general form's rows were measured in fp64)
    const int want = h->opt_group_lanes;
    if (want > 0 && built(want)) return want;
    // the measured best for this batch size (auto_table.h); where a row names a size that is not built, the next one down
    for (const AutoRow& r : kAutoTable) {
        if (r.form != form || r.dtype != dtype || r.horizon != H || n <= 0) continue;
        auto scaled = [&](int64_t at) { return at * h->cu_count / 256 < at ? at * h->cu_count / 256 : at; };
        int g = n < scaled(r.group8_below) ? 8 : (n < scaled(r.group4_below) ? 4 : 2);
        while (g > 2 && !built(g)) g /= 2;
        if (!built(g)) g = 4;
        return g;
    }
    return H == 40 ? 8 : (H == 10 ? 2 : 4);
}

// GROUP, kernels built for more than one wavefront per SIMD (fp32, compact form): does a batch of n take the full grid?
// From auto_table.h's pair_from: below it the longest instance sets the time and a lone wavefront iterates faster.
bool group_pair(const tpc_mpc_context* h, int H, int dtype, int64_t n, int form) {
    for (const AutoRow& r : kAutoTable) {
        if (r.form != form || r.dtype != dtype || r.horizon != H) continue;
        const int64_t at = r.pair_from * h->cu_count / 256 < r.pair_from ? r.pair_from * h->cu_count / 256 : r.pair_from;
        return n >= at;
    }
    return false;
}

// LANE needs enough instances to give every SIMD a full wavefront; below that WAVE's
// one-wavefront-per-instance launch finishes sooner.  Measured crossovers on MI355X
// (scripts/crossover.py, fp64, compact form, round 2 kernels; the chip has 65 536 LANE slots):
// fp32 at H = 4 and H = 10 (one instance per wavefront): between 24 576 and 32 768 instances; H = 20: WAVE still
// wins at 32 768, the largest batch its work queue takes (5.4 against 6.9 ms), and loses without the queue beyond.
// The WAVE kernel maps one decision variable to one lane, so it exists for I*H <= 64 only.
// Returns the kernel family to run, or -1 when WAVE was demanded for a shape it cannot take.
// `fma_ok`: the request is one the LANE_FMA family takes (compact form with usable bounds: fma_usable(); general form:
// fma_general_usable()); `compact`: the compact form (its WAVE / LANE_FMA crossovers were measured separately).
int pick_algo(const tpc_mpc_context* h, int algo, int I, int H, int64_t n, int dtype, bool fma_ok = false,
              bool compact = true, bool group_general = false) {
    if (!horizon_specialised(H)) return algo == TPC_MPC_ALGO_WAVE ? -1 : kAlgoGeneric;
    const bool wave_ok = I * H <= kWave || (I == 2 && H <= kWave);   // (two variables per lane past 64)
    const int lane = fma_ok ? TPC_MPC_ALGO_LANE_FMA : TPC_MPC_ALGO_LANE;   // the throughput family of AUTO
    if (algo == TPC_MPC_ALGO_WAVE) return wave_ok ? algo : -1;
    if (algo == TPC_MPC_ALGO_LANE) return algo;
    // LANE_FMA named at N = 30 / 40, compact form, fp64: GROUP (the same arithmetic, G lanes per instance) takes the request.
    // The one-lane kernels there parked their state in scratch around every refill pass -- 0.28 / 4.4 GB of HBM traffic per
    // 262 144-instance launch, 26x / 419x the algorithmic bytes -- and lost to GROUP at every batch size (43.9 against 54-56 ms
    // at N = 40); they are no longer built (mpc_ub_inst.hip).  fp32 keeps them (no spill), as does the exact-stop-test build
    // GROUP itself falls back on.
    if (algo == TPC_MPC_ALGO_LANE_FMA && compact && fma_ok && dtype == TPC_MPC_F64 && H >= 30 && group_lanes(h, H) > 0)
        return TPC_MPC_ALGO_GROUP;
    if (algo == TPC_MPC_ALGO_LANE_FMA) return lane;
    // GROUP is LANE_FMA's arithmetic with G lanes per instance: the same requests, the horizons a group divides
    if (algo == TPC_MPC_ALGO_GROUP) return (compact ? (fma_ok && group_lanes(h, H) > 0) : group_general) ? algo : lane;
    const int64_t lanes = (int64_t)h->cu_count * 4 * kWave;
    // (N = 40 with two inputs: the two-variables-per-lane WAVE kernel against a LANE pass that lasts as long
    // as its slowest instance, 50 ms whatever the batch: 42.0 against 50.0 ms at 16 384, 62.4 against 49.9 at 24 576)
    // (fp64 with at most 32 variables: two instances per wavefront over the work queue -- WAVE wins up to the
    // largest batch the queue takes: 0.65 against 1.00 ms at 32 768 x N = 10, 0.20 against 0.21 at N = 4;
    // without the queue, at 49 152, it loses 1.6 to 1.0)
    const bool paired = dtype == TPC_MPC_F64 && I * H <= kWave / 2;
    // (the queue's crossover was measured on a 256-CU part; a smaller one -- a CPX partition -- scales it down)
    const int64_t queue_cross = (kWaveQueueMaxInstances * h->cu_count / 256 < kWaveQueueMaxInstances
                                     ? kWaveQueueMaxInstances * h->cu_count / 256 : kWaveQueueMaxInstances) + 1;
    // (N = 40, two inputs: a LANE pass lasts as long as its slowest instance whatever the batch -- 10 000 iterations of
    // 5.1 us in the bit-exact family, 2.9 us in LANE_FMA: 51 / 29.5 ms -- and the two-variables-per-lane WAVE kernel
    // with dense Hessian rows (the general form) takes 2.6 us per instance: 42 ms at 16 384.  So WAVE up to 19 456
    // instances against LANE ...)
    // ... and the compact model's WAVE kernel at N = 40 builds its gradient from prefix sums (mpc_wave.h,
    // scan_gradient): 0.92 us per instance through the queue, 15 ms at 16 384 -- ahead of either LANE family up to
    // the largest batch the queue takes.
    const int64_t two_per_lane_cross = (fma_ok && compact) ? queue_cross : lanes * 19 / 64;
    int64_t crossover = I * H > kWave ? two_per_lane_cross
                        : ((H >= 20 || paired) ? queue_cross : lanes * 7 / 16);
    if (fma_ok && compact) {
        // compact form: WAVE, then GROUP with fewer and fewer lanes per instance, then LANE_FMA, at crossovers measured
        // per dtype and horizon (auto_table.h, generated by scripts/measure_crossover.py; profiles/r04_crossover.txt).
        // N = 4 and 5 have no GROUP kernels (profiles/r03_crossover.txt: WAVE up to 28 672 in fp64, 24 576 / 21 504 in fp32).
        const bool d = dtype == TPC_MPC_F64;
        auto scaled = [&](int64_t at) { return at * h->cu_count / 256 < at ? at * h->cu_count / 256 : at; };
        for (const AutoRow& r : kAutoTable) {
            if (r.form != 0 || r.dtype != dtype || r.horizon != H) continue;
            if (n < scaled(r.wave_below) && n <= kWaveQueueMaxInstances) return TPC_MPC_ALGO_WAVE;
            if (n < scaled(r.group2_below)) return TPC_MPC_ALGO_GROUP;
            return lane;
        }
        int64_t at = kWaveQueueMaxInstances + 1;
        if (d && (H == 4 || H == 5)) at = 28672;
        if (!d && H == 4) at = 24576;
        if (!d && H == 5) at = 21504;
        crossover = scaled(at);
    }
    if (!compact && group_general) {
        // general form with group kernels: the same three-way split, from the rows measured for it (two inputs, fp64)
        auto scaled = [&](int64_t at) { return at * h->cu_count / 256 < at ? at * h->cu_count / 256 : at; };
        for (const AutoRow& r : kAutoTable) {
            if (r.form != 1 || r.horizon != H) continue;
            if (wave_ok && n < scaled(r.wave_below) && n <= kWaveQueueMaxInstances) return TPC_MPC_ALGO_WAVE;
            if (n < scaled(r.group2_below)) return TPC_MPC_ALGO_GROUP;
            return lane;
        }
    }
    return (n >= crossover || !wave_ok) ? lane : TPC_MPC_ALGO_WAVE;
}

// The unit-box coordinates of the LANE_FMA family need a box: finite bounds with upper > lower (dlib
// also accepts upper == lower, a pinned input: that goes to LANE).
bool fma_usable(const tpc_mpc_params* p) {
    for (int j = 0; j < 2; ++j)
        if (!(std::isfinite(p->lower[j]) && std::isfinite(p->upper[j]) && p->upper[j] > p->lower[j])) return false;
    return true;
}

// A compact request whose coordinate-descent phase can meet an arg-max (mpc.h:289-309) that is a TIE in exact arithmetic.
// With weight_phi == 0 the heading enters the cost through the position alone, and dlib's coordinate step divides by
// Q_diag, which leaves R out (mpc.h:324): after a step on u[0](0) from the cold start the Q part of that component is
// zero exactly (c N1[0] = 0), the predicted error is still linear in the step index (every later control is 0:
// E[k] = E0 + k d), and for N = 3m - 1 the partial sum N0[m] = q0 sum_{k >= m} E[k] is a multiple of N1[0] and vanishes
// with it -- df[m-1](0), df[m](0) and -df[m](1) are then one real number, the extremum of the first input's
// components and, for part of the speed range, of the whole gradient; computed, they differ in their last bits
// only (N = 5: m = 2, traced in NOTEBOOK.md).  dlib's strict '>' takes whichever its own rounding left
// largest; another operation order takes another one, both valid descent steps, and the two paths part for good
// (N = 5, reversing at |T v| ~ 0.21 .. 0.31: 2 % of a batch, |du| up to 1.3e-3; other ties of the same origin at
// N = 6).  Not a rounding-of-eps event, so the tolerance families' statement does not cover it: AUTO sends such
// requests to the bit-exact kernels.
// How small is "zero".  A weight_phi > 0 moves the three components apart by about weight_phi / weight_y of their
// size (the heading's terms against the position's, states and model entries being O(0.1 .. 1)); the families'
// rounding moves them by ~1e-14 of it.  Measured on the batch of tests/test_vehicles_host.py (3000 reversing instances,
// weight_y = 20): weight_phi / weight_y = 5e-22 parts 82 solves like 0 does, 1e-16: 65, 1e-14: 1, 1e-12 and every
// larger ratio up to 1e-3: none.  The threshold is 2^-30 (9e-10): three decades above the last ratio that showed.
bool cd_tie_prone(const tpc_mpc_params* p) {
    return p->weight_phi <= p->weight_y * 0x1p-30 && p->smo_iters > 0 && p->max_iter > 0;
}

// General form, GROUP (mpc_groupg_inst.hip): N = 10, 20, 30, 40; fp32 only where the general-form LANE_FMA unit stands
// in front of it (cold starts at N <= 20), fp64 also with the controller state in or out and at N = 30, 40.
bool group_general_usable(int dtype, int H, const void* controls, const void* v) {
    if (H != 10 && H != 20 && H != 30 && H != 40) return false;
    const bool via_lane = controls || v || H > 20;
    return !via_lane || dtype == TPC_MPC_F64;
}

// General form: the LANE_FMA kernels exist for N <= 20 and start cold (the controller state in or out is LANE's).
bool fma_general_usable(int H, const void* controls, const void* v) {
    return (H == 4 || H == 5 || H == 10 || H == 20) && !controls && !v;
}

int64_t lane_rec_len(int H, int dtype) {
    switch (H) {
#define X(h) case h: return lane_rec_len_h##h(dtype);
        X(4) X(5) X(10) X(20) X(30) X(40)
#undef X
    }
    return 0;
}

// the generic kernel is one launch: bracket it with the profiling events like the WAVE launcher does
template <class Launch> hipError_t generic_launch(const Workspace& ws, hipStream_t s, Launch launch) {
    if (ws.ev) (void)hipEventRecord(ws.ev[0], s);
    const hipError_t e = launch();
    if (ws.ev) { (void)hipEventRecord(ws.ev[1], s); (void)hipEventRecord(ws.ev[2], s); }
    return e;
}

hipError_t dispatch_compact(int algo, int H, int dtype, const CompactArgs& a, const Knobs& k,
                            const Workspace& ws, hipStream_t s) {
    if (algo == kAlgoGeneric) return generic_launch(ws, s, [&] { return generic_compact(dtype, H, a, k, ws.state, s); });
    if (algo == TPC_MPC_ALGO_LANE_FMA || algo == TPC_MPC_ALGO_GROUP) {
        // (compared in the arithmetic type: the kernels see the bounds rounded to it)
        const bool eqb = dtype == TPC_MPC_F64 ? (a.lo[0] == a.lo[1] && a.hi[0] == a.hi[1])
                                              : ((float)a.lo[0] == (float)a.lo[1] && (float)a.hi[0] == (float)a.hi[1]);
        if (algo == TPC_MPC_ALGO_GROUP) {
            switch (H) {
#define X(h) case h: return group_compact_h##h(dtype, eqb ? 1 : 0, ws.group_lanes, a, k, ws, s);
                X(10) X(20) X(30) X(40)
#undef X
            }
            return hipErrorInvalidValue;
        }
        switch (H) {
#define X(h) case h: return ub_compact_h##h(dtype, eqb ? 1 : 0, a, k, ws, s);
            X(4) X(5) X(10) X(20) X(30) X(40)
#undef X
        }
        return hipErrorInvalidValue;
    }
    switch (H) {
#define X(h) case h: return algo == TPC_MPC_ALGO_LANE ? lane_compact_h##h(dtype, a, k, ws, s) \
                                                       : wave_compact_h##h(dtype, a, k, ws, s);
        X(4) X(5) X(10) X(20) X(30) X(40)
#undef X
    }
    return hipErrorInvalidValue;
}
hipError_t dispatch_general(int algo, int I, int H, int dtype, const GeneralArgs& a, const Knobs& k,
                            const Workspace& ws, hipStream_t s) {
    if (algo == kAlgoGeneric) return generic_launch(ws, s, [&] { return generic_general(dtype, I, H, a, k, ws.state, s); });
    if (algo == TPC_MPC_ALGO_GROUP) {
        switch (H) {
#define X(h) case h: return groupg_general_h##h(dtype, I, ws.group_lanes, a, k, ws, s);
            X(10) X(20) X(30) X(40)
#undef X
        }
        return hipErrorInvalidValue;
    }
    if (algo == TPC_MPC_ALGO_LANE_FMA) {
        switch (H) {
#define X(h) case h: return ub_general_h##h(dtype, I, a, k, ws, s);
            X(4) X(5) X(10) X(20)
#undef X
        }
        return hipErrorInvalidValue;
    }
    switch (H) {
#define X(h) case h: return algo == TPC_MPC_ALGO_LANE ? lane_general_h##h(dtype, I, a, k, ws, s) \
                                                       : wave_general_h##h(dtype, I, a, k, ws, s);
        X(4) X(5) X(10) X(20) X(30) X(40)
#undef X
    }
    return hipErrorInvalidValue;
}

// AUTO's parity guarantee (include/tpc_mpc.h): where AUTO picked a tolerance family, the instances that family left on
// the iteration cap are solved once more by the bit-exact LANE arithmetic and published with dlib's bits.  fp64, the
// specialised horizons, cold starts; a host opts out with TPC_MPC_PARAM_FAST_CAPPED.
bool wants_cap_resolve(const tpc_mpc_params* p, int algo_ran) {
    return p->algo == TPC_MPC_ALGO_AUTO && p->dtype == TPC_MPC_F64 && p->max_iter > 0 &&
           (p->options & TPC_MPC_PARAM_FAST_CAPPED) == 0 && horizon_specialised(p->horizon) &&
           (algo_ran == TPC_MPC_ALGO_WAVE || algo_ran == TPC_MPC_ALGO_LANE_FMA || algo_ran == TPC_MPC_ALGO_GROUP);
}
// where the first pass leaves its iteration counts when the caller did not ask for them
int cap_iters_buffer(tpc_mpc_context* h, int64_t n, int32_t** out) {
    int rc = ensure(h, &h->cap_iters, &h->cap_iters_bytes, pad256(n * 4));
    if (rc) return rc;
    *out = (int32_t*)h->cap_iters;
    return TPC_MPC_OK;
}
hipError_t resolve_compact(int H, const CompactArgs& a, const Knobs& k, const Workspace& ws, hipStream_t s, double presolved_from = 0.0,
                           const uint32_t* pre_len = nullptr, uint32_t pre_limit = 0u) {
    switch (H) {
#define X(h) case h: return lane_resolve_compact_h##h(a, k, ws, a.iters, a.flags, s, presolved_from, pre_len, pre_limit);
        X(4) X(5) X(10) X(20) X(30) X(40)
#undef X
    }
    return hipErrorInvalidValue;
}
hipError_t resolve_general(int I, int H, const GeneralArgs& a, const Knobs& k, const Workspace& ws, hipStream_t s,
                           double presolved_from = 0.0, const uint32_t* pre_len = nullptr, uint32_t pre_limit = 0u) {
    switch (H) {
#define X(h) case h: return lane_resolve_general_h##h(I, a, k, ws, a.iters, a.flags, s, presolved_from, pre_len, pre_limit);
        X(4) X(5) X(10) X(20) X(30) X(40)
#undef X
    }
    return hipErrorInvalidValue;
}

int prepare_workspace(tpc_mpc_context* h, int algo, int H, int dtype, int64_t n, Workspace* ws, int form = 0) {
    ws->state = nullptr;
    ws->ticket = h->ws_words;
    ws->stats = (unsigned long long*)(h->ws_words + 4);
    ws->capacity_bytes = 0;
    ws->ev = h->profiling ? h->ev : nullptr;
    ws->wave_group = h->opt_wave_group;
    ws->group_lanes = group_lanes(h, H, dtype, n, form);
    ws->max_waves = h->max_waves;
    if (h->pre_busy && h->pre_group_waves > 0 && (ws->max_waves == 0 || ws->max_waves > h->pre_group_waves))
        ws->max_waves = h->pre_group_waves;   // a presolve holds the other SIMDs (presolve_begin)
    ws->group_pair = group_pair(h, H, dtype, n, form);
    ws->lanex_below = h->opt_lanex_below;
    ws->cu_count = h->cu_count;
    h->ev_valid = h->profiling;
    h->last_algo = algo;
    ws->keys = ws->rank = ws->order = nullptr;
    ws->sort_temp = nullptr;
    ws->sort_temp_bytes = 0;
    if (algo == kAlgoGeneric) {
        int rc = ensure(h, &h->ws_state, &h->ws_bytes, pad256(generic_scratch_bytes(H, dtype, n)));
        if (rc) return rc;
        ws->state = h->ws_state;
        ws->capacity_bytes = h->ws_bytes;
    }
    if (algo == TPC_MPC_ALGO_WAVE) {
        // order[] of the longest-first queue (mpc_wave.h); batches that fit the chip at once do not use it
        // + its ticket words, one cache line each (kQueueTickets x 256 B)
        int rc = ensure(h, &h->ws_state, &h->ws_bytes, pad256(n * 4) + kQueueTicketBytes);
        if (rc) return rc;
        ws->order = (uint32_t*)h->ws_state;
        ws->ticket = (uint32_t*)((char*)h->ws_state + pad256(n * 4));
        ws->capacity_bytes = h->ws_bytes;
    }
    if (algo == TPC_MPC_ALGO_LANE || algo == TPC_MPC_ALGO_LANE_FMA || algo == TPC_MPC_ALGO_GROUP) {
        // records | keys | rank | order | counting-sort bins
        const int64_t rec_b = pad256(lane_rec_len(H, dtype) * (int64_t)esize(dtype) * n);
        const int64_t col_b = pad256(n * 4);
        const size_t tmp_b = sort_temp_bytes(n);
        int rc = ensure(h, &h->ws_state, &h->ws_bytes, rec_b + 3 * col_b + pad256((int64_t)tmp_b));
        if (rc) return rc;
        char* b = (char*)h->ws_state;
        ws->state = b;
        ws->keys = (uint32_t*)(b + rec_b);
        ws->rank = (uint32_t*)(b + rec_b + col_b);
        ws->order = (uint32_t*)(b + rec_b + 2 * col_b);
        ws->sort_temp = b + rec_b + 3 * col_b;
        ws->sort_temp_bytes = tmp_b;
        ws->capacity_bytes = h->ws_bytes;
    }
    return TPC_MPC_OK;
}

// Workspace of the re-solve of capped instances (the LANE layout in the handle's scratch).  resolve_reserve() grows the
// scratch BEFORE the first pass is launched -- growing frees, and nothing may be freed under a running kernel's feet --
// resolve_workspace() carves it afterwards; ticket, statistics and events of the first pass stay what they are
// (tpc_mpc_last_lane_stats / _kernel_times describe the family that solved the batch).
int resolve_reserve(tpc_mpc_context* h, int H, int dtype, int64_t n) { return reserve_lane_workspace(h, H, dtype, n); }
int resolve_workspace(tpc_mpc_context* h, int H, int dtype, int64_t n, Workspace* ws) {
    const bool ev_valid = h->ev_valid;
    const int last_algo = h->last_algo;
    const int rc = prepare_workspace(h, TPC_MPC_ALGO_LANE, H, dtype, n, ws);
    h->ev_valid = ev_valid;
    h->last_algo = last_algo;
    ws->ev = nullptr;
    ws->ticket = h->ws_words + 16;   // ticket | queue length | statistics: 32 contiguous bytes (mpc_lane_inst.hip, resolve)
    ws->stats = (unsigned long long*)(h->ws_words + 18);
    return rc;
}

// Copy `rows` rows of `width` bytes between arrays of different leading dimensions (pitches in bytes).
hipError_t copy_rows(void* dst, int64_t dpitch, const void* src, int64_t spitch, int64_t width, int64_t rows,
                     hipMemcpyKind kind, hipStream_t s) {
    if (rows <= 0 || width <= 0) return hipSuccess;
    if (rows == 1 || (dpitch == width && spitch == width))   // one run of bytes
        return hipMemcpyAsync(dst, src, (size_t)(width * rows), kind, s);
    return hipMemcpy2DAsync(dst, (size_t)dpitch, src, (size_t)spitch, (size_t)width, (size_t)rows, kind, s);
}

int check_general_io(tpc_mpc_context* h, const tpc_mpc_general_io* io, int mem) {
    if (!io) return fail(h, TPC_MPC_ERR_BAD_ARG, "null io");
    if (io->inputs != 1 && io->inputs != 2) return fail(h, TPC_MPC_ERR_BAD_ARG, "inputs must be 1 or 2");
    if (io->n < 0 || io->ld < io->n || io->n > 0x7fffffffll)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "need 0 <= n <= ld, n < 2^31");
    if (mem != TPC_MPC_HOST && mem != TPC_MPC_DEVICE) return fail(h, TPC_MPC_ERR_BAD_ARG, "bad memory kind");
    return TPC_MPC_OK;
}

// Checks that several general-form entries make.  Each entry calls them where its own checks need them: the order in
// which an entry's checks fire is part of its behaviour (a host-only handle reports argument errors before NO_DEVICE).
// The model's nine arrays (`also`: whether the entry's own required array is there as well)
int check_model(tpc_mpc_context* h, const tpc_mpc_general_io* io, bool also = true) {
    if (!io->A || !io->B || !io->C || !io->Q || !io->R || !io->lower || !io->upper || !io->x0 || !io->targets || !also)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
    return TPC_MPC_OK;
}
int check_polish(tpc_mpc_context* h, const tpc_mpc_polish* q) {
    if (!q) return fail(h, TPC_MPC_ERR_BAD_ARG, "null polish struct");
    if (!(q->tol > 0.0) || q->max_rounds < 0)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "polish needs tol > 0 and max_rounds >= 0");
    return TPC_MPC_OK;
}
int check_steps(tpc_mpc_context* h, int32_t steps) {
    if (steps < 0 || steps > (1 << 24)) return fail(h, TPC_MPC_ERR_BAD_ARG, "need 0 <= steps <= 2^24");
    return TPC_MPC_OK;
}
int check_fallback(tpc_mpc_context* h, int32_t fallback) {
    if (fallback != TPC_MPC_NEWTON_FALLBACK_SOLVE && fallback != TPC_MPC_NEWTON_FALLBACK_NONE)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "unknown fallback %d", (int)fallback);
    return TPC_MPC_OK;
}
// (what an entry named `entry` returns for p->dtype != TPC_MPC_F64)
int fp64_only(tpc_mpc_context* h, const char* entry) {
    return fail(h, TPC_MPC_ERR_BAD_ARG, "%s is fp64 only: p->dtype must be TPC_MPC_F64", entry);
}
// the batch size and memory kind of the compact entries (check_general_io makes these checks for an io)
int check_batch(tpc_mpc_context* h, int64_t n, int mem) {
    if (n < 0 || n > 0x7fffffffll) return fail(h, TPC_MPC_ERR_BAD_ARG, "need 0 <= n < 2^31");
    if (mem != TPC_MPC_HOST && mem != TPC_MPC_DEVICE) return fail(h, TPC_MPC_ERR_BAD_ARG, "bad memory kind");
    return TPC_MPC_OK;
}
// what a host-only handle refuses of the Newton-first entries: the fallback solve, and DEVICE memory
int check_host_only_newton(tpc_mpc_context* h, bool solve, int mem) {
    if (h->host_only && solve)
        return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle (TPC_MPC_DEVICE_NONE): the fallback solve runs on the device only; use TPC_MPC_NEWTON_FALLBACK_NONE");
    if (h->host_only && mem == TPC_MPC_DEVICE)
        return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle (TPC_MPC_DEVICE_NONE): HOST memory only");
    return TPC_MPC_OK;
}
// ... and of a one-launch pass ("backward pass", "forward pass", "polish"): DEVICE memory
int check_host_only_pass(tpc_mpc_context* h, int mem, const char* pass) {
    if (h->host_only && mem == TPC_MPC_DEVICE)
        return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle (TPC_MPC_DEVICE_NONE): the %s takes HOST memory only", pass);
    return TPC_MPC_OK;
}
// what a compact backward pass returns for an empty batch (or no steps): zero shared-parameter gradients, in `mem`
int zero_dparams(tpc_mpc_context* h, void* dparams, int count, uint32_t* flags_out, int mem, void* stream) {
    if (dparams) {
        if (mem == TPC_MPC_HOST) {
            std::memset(dparams, 0, (size_t)count * 8);
        } else {
            HIP_TRY(h, hipSetDevice(h->device));
            HIP_TRY(h, hipMemsetAsync(dparams, 0, (size_t)count * 8, (hipStream_t)stream));
        }
    }
    if (flags_out) *flags_out = 0;
    return TPC_MPC_OK;
}
// the ten model values of the compact form into the Args of the exact solve or its backward pass
template <class Args> void bind_compact_model(Args* a, const tpc_mpc_params* p) {
    a->T = p->step_size; a->l = p->wheelbase; a->q0 = p->weight_y; a->q1 = p->weight_phi;
    a->r[0] = p->weight_steering_front; a->r[1] = p->weight_steering_rear;
    for (int j = 0; j < 2; ++j) { a->lo[j] = p->lower[j]; a->hi[j] = p->upper[j]; }
}

}  // namespace

namespace tpc {

// The family a compact request asks for.  AUTO's guarantee (include/tpc_mpc.h) covers fp64: there a request whose
// coordinate-descent phase can tie (cd_tie_prone) is LANE's, whatever its size -- the one-instance entry included.
int compact_algo(const tpc_mpc_params* p) {
    return p->algo == TPC_MPC_ALGO_AUTO && p->dtype == TPC_MPC_F64 && cd_tie_prone(p) ? TPC_MPC_ALGO_LANE : p->algo;
}

// A bin of a mixed-horizon batch that the GROUP family takes (tpc_mpc_mixed.hip runs those side by side, each on its
// share of the SIMDs): AUTO or GROUP asked for, bounds the unit box can take, a horizon with group kernels.
bool group_applicable(const tpc_mpc_context* h, const tpc_mpc_params* p, int H) {
    const int algo = compact_algo(p);
    return (algo == TPC_MPC_ALGO_AUTO || algo == TPC_MPC_ALGO_GROUP) && fma_usable(p) && group_lanes(h, H) > 0;
}

// `host_ok`: the entry point also serves a host-only handle (tpc_mpc_solve_one); every other one needs the device
int check_common(tpc_mpc_context* h, const tpc_mpc_params* p, bool host_ok) {
    if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
    if (h->host_only && !host_ok)
        return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle (TPC_MPC_DEVICE_NONE): only tpc_mpc_solve_one is served");
    if (!p) return fail(h, TPC_MPC_ERR_BAD_ARG, "null params");
    if (!horizon_ok(p->horizon))
        return fail(h, TPC_MPC_ERR_BAD_HORIZON, "horizon %d outside 1 .. %d", p->horizon, kMaxHorizon);
    if (p->dtype != TPC_MPC_F64 && p->dtype != TPC_MPC_F32) return fail(h, TPC_MPC_ERR_BAD_ARG, "bad dtype");
    if (p->algo < TPC_MPC_ALGO_AUTO || p->algo > TPC_MPC_ALGO_GROUP) return fail(h, TPC_MPC_ERR_BAD_ARG, "bad algo");
    if (!(p->eps > 0)) return fail(h, TPC_MPC_ERR_BAD_EPS, "eps must be > 0 (mpc.h:202)");
    if (p->options & ~TPC_MPC_PARAM_FAST_CAPPED) return fail(h, TPC_MPC_ERR_BAD_ARG, "unknown bits in tpc_mpc_params.options");
    if (p->max_iter > 0x7fffffffull || p->smo_iters > 0x7fffffffull)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "max_iter / smo_iters must fit in 31 bits");
    return TPC_MPC_OK;
}

// mpc_abstract.h:90-97: min(Q) >= 0, min(R) > 0, min(upper-lower) >= 0
int check_compact_model(tpc_mpc_context* h, const tpc_mpc_params* p) {
    if (!(p->weight_y >= 0) || !(p->weight_phi >= 0))
        return fail(h, TPC_MPC_ERR_BAD_WEIGHTS, "min(Q) >= 0 violated (mpc_abstract.h:90-97)");
    if (!(p->weight_steering_front > 0) || !(p->weight_steering_rear > 0))
        return fail(h, TPC_MPC_ERR_BAD_WEIGHTS, "min(R) > 0 violated (mpc_abstract.h:90-97)");
    for (int j = 0; j < 2; ++j)
        if (!(p->upper[j] >= p->lower[j]))
            return fail(h, TPC_MPC_ERR_BAD_BOUNDS, "upper >= lower violated (mpc_abstract.h:90-97)");
    if (!std::isfinite(p->step_size) || !std::isfinite(p->wheelbase) || p->wheelbase == 0)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "step_size / wheelbase must be finite, wheelbase != 0");
    return TPC_MPC_OK;
}

// StreamOrder.  Solves of one handle share its scratch (ticket, flag word, statistics, records,
// queue, staging), so two of them must never overlap.  On one stream they cannot; a solve that
// arrives on a different stream than the previous one first makes its stream wait for the event
// recorded behind that previous solve.
int stream_order_begin(tpc_mpc_context* h, hipStream_t s) {
    if (h->have_last && h->last_stream != s) HIP_TRY(h, hipStreamWaitEvent(s, h->done_ev, 0));
    return TPC_MPC_OK;
}
int stream_order_end(tpc_mpc_context* h, hipStream_t s) {
    HIP_TRY(h, hipEventRecord(h->done_ev, s));
    h->last_stream = s;
    h->have_last = true;
    return TPC_MPC_OK;
}

int finish_flags(tpc_mpc_context* h, uint32_t* flags_out, hipStream_t s) {
    if (!flags_out) return TPC_MPC_OK;
    uint32_t f = 0;
    HIP_TRY(h, hipMemcpyAsync(&f, h->ws_words + 1, sizeof(f), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    *flags_out = f;
    return TPC_MPC_OK;
}

int reserve_lane_workspace(tpc_mpc_context* h, int H, int dtype, int64_t n) {
    const bool ev_valid = h->ev_valid;
    const int last_algo = h->last_algo;
    Workspace ws;
    const int rc = prepare_workspace(h, horizon_specialised(H) ? TPC_MPC_ALGO_LANE : kAlgoGeneric, H, dtype, n, &ws);
    h->ev_valid = ev_valid;
    h->last_algo = last_algo;
    return rc;
}

int context_new(int device, int cu_count, tpc_mpc_context** out) {
    tpc_mpc_context* h = new (std::nothrow) tpc_mpc_context;
    if (!h) return fail(nullptr, TPC_MPC_ERR_ALLOC, "out of host memory");
    h->device = device;
    h->cu_count = cu_count;
    h->device_cu_count = cu_count;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void**)&h->ws_words, 128);
    if (e == hipSuccess) e = hipMemset(h->ws_words, 0, 128);
    if (e == hipSuccess) e = hipHostMalloc(&h->pin_host, 512, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&h->pin_dev, h->pin_host, 0);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->done_ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)tpc_mpc_destroy(h);
        return fail(nullptr, TPC_MPC_ERR_HIP, "create: %s", hipGetErrorString(e));
    }
    std::memset(h->pin_host, 0, 512);
    *out = h;
    return TPC_MPC_OK;
}

// The general form on DEVICE arrays, launches only (the sharded entry, tpc_mpc_comm.cpp, brackets it with the stream
// order, the flag word and the exchange): io describes the block to solve.
static double presolve_lambda(const tpc_mpc_params* p);
// AUTO's presolve (see presolve_begin below): scratch of its own in the LANE layout, `side_bytes` behind it, the side
// stream and its events
static int presolve_scratch(tpc_mpc_context* h, int H, int dtype, int64_t n, int64_t side_bytes, Workspace* ws, char** side) {
    const int64_t rec_b = pad256(lane_rec_len(H, dtype) * (int64_t)esize(dtype) * n), col_b = pad256(n * 4);
    const size_t tmp_b = sort_temp_bytes(n);
    const int64_t lane_b = rec_b + 3 * col_b + pad256((int64_t)tmp_b);
    int rc = ensure(h, &h->pre, &h->pre_bytes, lane_b + side_bytes);
    if (rc) return rc;
    if (!h->pre_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->pre_stream, hipStreamNonBlocking));
    if (!h->pre_fork) HIP_TRY(h, hipEventCreateWithFlags(&h->pre_fork, hipEventDisableTiming));
    if (!h->pre_done) HIP_TRY(h, hipEventCreateWithFlags(&h->pre_done, hipEventDisableTiming));
    char* b = (char*)h->pre;
    std::memset(ws, 0, sizeof(*ws));
    ws->state = b;
    ws->keys = (uint32_t*)(b + rec_b);
    ws->rank = (uint32_t*)(b + rec_b + col_b);
    ws->order = (uint32_t*)(b + rec_b + 2 * col_b);
    ws->sort_temp = b + rec_b + 3 * col_b;
    ws->sort_temp_bytes = tmp_b;
    ws->capacity_bytes = lane_b;
    ws->ev = nullptr;
    ws->lanex_below = h->opt_lanex_below;
    ws->cu_count = h->cu_count;
    ws->ticket = h->ws_words + 24;   // ticket | queue length | statistics: 32 contiguous bytes, as the second pass's (resolve_workspace)
    ws->stats = (unsigned long long*)(h->ws_words + 26);
    *side = b + lane_b;
    return TPC_MPC_OK;
}
// the share of the chip a presolve takes (see presolve_begin): false = this batch is not tried
static bool presolve_share(tpc_mpc_context* h, int64_t n, Presolve* ps) {
    const int simds = (h->device_cu_count > 0 ? h->device_cu_count : 256) * 4;
    const int solo_waves = simds * 7 / 16;
    if (n > (int64_t)solo_waves * 8 * 5) return false;
    ps->limit = (uint32_t)solo_waves * 8u;
    ps->group_waves = simds - solo_waves;
    return true;
}

int general_launch(tpc_mpc_context* h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, hipStream_t s) {
    const int I = io->inputs, H = p->horizon;
    const int64_t n = io->n;
    const int algo = pick_algo(h, p->algo, I, H, n, p->dtype, fma_general_usable(H, io->controls_inout, io->v_inout), false,
                                   group_general_usable(p->dtype, H, io->controls_inout, io->v_inout));
    if (algo < 0) return fail(h, TPC_MPC_ERR_BAD_HORIZON, "the WAVE kernel exists for the specialised horizons with inputs*horizon <= 64 only; use LANE or AUTO");
    GeneralArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n = n; a.ld = io->ld; a.shift_controls = 1;
    a.A = io->A; a.B = io->B; a.C = io->C; a.Q = io->Q; a.R = io->R; a.lo = io->lower; a.hi = io->upper;
    a.x0 = io->x0; a.targets = io->targets; a.controls = io->controls_inout; a.v = io->v_inout;
    a.u0 = io->u0; a.iters = io->iters;
    a.flags = h->ws_words + 1;
    a.work_hint = take_hint(h, n);
    const bool fix = wants_cap_resolve(p, algo) && !a.controls && !a.v;
    int rc = TPC_MPC_OK;
    if (fix && !a.iters) rc = cap_iters_buffer(h, n, &a.iters);
    if (!rc && fix) rc = resolve_reserve(h, H, p->dtype, n);
    if (rc) return rc;
    // AUTO's presolve, as the compact form's (presolve_begin): side outputs = I rows of u0 and the iteration counts
    Presolve ps;
    const double lf = presolve_lambda(p);
    const int64_t ubytes = pad256((int64_t)I * a.ld * 8);   // (the kernels address row j at u0 + j * ld: the side rows keep the caller's ld)
    if (fix && algo == TPC_MPC_ALGO_GROUP && lf > 0.0 && !h->pre_busy && presolve_share(h, n, &ps)) {
        Workspace wp;
        char* side = nullptr;
        rc = presolve_scratch(h, H, p->dtype, n, ubytes + pad256(n * 4), &wp, &side);
        if (rc) return rc;
        GeneralArgs a2 = a;
        a2.u0 = side;
        a2.iters = (int32_t*)(side + ubytes);
        a2.work_hint = nullptr;
        ps.side_front = side;
        ps.side_iters = a2.iters;
        ps.queue = wp.order;
        ps.queue_len = wp.ticket + 1;
        ps.lambda_from = lf;
        HIP_TRY(h, hipEventRecord(h->pre_fork, s));
        HIP_TRY(h, hipStreamWaitEvent(h->pre_stream, h->pre_fork, 0));
        ps.on = true;
        h->pre_busy = true;
        h->pre_group_waves = ps.group_waves;
        hipError_t e = hipErrorInvalidValue;
        switch (H) {
#define X(hh) case hh: e = lane_presolve_general_h##hh(I, a2, knobs_of(p), wp, lf, ps.limit, h->pre_stream); break;
            X(4) X(5) X(10) X(20) X(30) X(40)
#undef X
        }
        if (e != hipSuccess) {
            h->pre_busy = false;
            (void)hipEventRecord(h->pre_done, h->pre_stream);
            (void)hipStreamWaitEvent(s, h->pre_done, 0);
            return hip_fail(h, e, "kernel launch (presolve)");
        }
    }
    auto join = [&]() {
        if (!ps.on) return;
        ps.on = false;
        h->pre_busy = false;
        (void)hipEventRecord(h->pre_done, h->pre_stream);
        (void)hipStreamWaitEvent(s, h->pre_done, 0);
    };
    Workspace ws;
    rc = prepare_workspace(h, algo, H, p->dtype, n, &ws, 1);
    if (rc) { join(); return rc; }
    hipError_t e = dispatch_general(algo, I, H, p->dtype, a, knobs_of(p), ws, s);
    join();
    if (e == hipSuccess && ps.lambda_from > 0.0)
        e = presolve_merge_rows(ps.queue, ps.queue_len, n, ps.side_front, ps.side_iters, a.u0, a.iters, I, a.ld, ps.limit, s);
    if (e == hipSuccess && fix) {
        Workspace ws2;
        rc = resolve_workspace(h, H, p->dtype, n, &ws2);
        if (rc) return rc;
        e = resolve_general(I, H, a, knobs_of(p), ws2, s, ps.lambda_from, ps.queue_len, ps.limit);
    }
    if (e != hipSuccess) return hip_fail(h, e, "kernel launch");
    return TPC_MPC_OK;
}
int check_general_device_io(tpc_mpc_context* h, const tpc_mpc_general_io* io) {
    int rc = check_general_io(h, io, TPC_MPC_DEVICE);
    if (rc) return rc;
    return io->n > 0 ? check_model(h, io, io->u0 != nullptr) : TPC_MPC_OK;
}

static void compact_args(tpc_mpc_context* h, const tpc_mpc_params* p, int64_t n, const void* v, const void* dy, const void* dphi,
                         void* front, void* rear, int32_t* iters, CompactArgs* a) {
    std::memset(a, 0, sizeof(*a));
    a->n = n;
    a->v = v; a->dy = dy; a->dphi = dphi;
    a->front = front; a->rear = rear; a->iters = iters;
    a->flags = h->collect_flags ? h->ws_words + 1 : nullptr;
    a->step = p->step_size; a->wheelbase = p->wheelbase;
    a->q[0] = p->weight_y; a->q[1] = p->weight_phi;
    a->r[0] = p->weight_steering_front; a->r[1] = p->weight_steering_rear;
    a->lo[0] = p->lower[0]; a->lo[1] = p->lower[1]; a->hi[0] = p->upper[0]; a->hi[1] = p->upper[1];
}

// Which instances will end on the iteration cap can be said before any of them is solved: dlib's iteration count grows like
// 5.5 sqrt(lambda) (lambda = its trace bound of the Hessian, mpc.h:116-123; measured with the checker on the synthetic
// streams: median 5.45; 6.36 at most among the instances near the cap at N = 40), so lambda >= (max_iter / 7)^2 names them --
// at N = 40 with dlib's default cap: every one of the 1 614 capped instances of a 16 384-instance batch, 20 % of the batch,
// half of those really capped.  The margin matters: ONE capped instance the prediction misses costs the second pass its
// whole 10 000-iteration chain again (with max_iter / 6.25 one of 16 384 slipped through: 31 ms instead of 16).  Still a
// prediction, not a decision: an instance it takes comes back with dlib's bits whether it capped or not, one it misses is
// caught by the flag-driven second pass as before.  Horizons below 30 never get near the cap with dlib's defaults and
// (and N = 30: lambda <= 1.1e6 at 4 m/s) are left alone: a presolve that finds nothing still costs GROUP its share of the chip.
// No presolve when smo_iters >= max_iter: every instance then ends inside the coordinate-descent phase, where nothing is
// queued and so nothing merged, while the second pass would still skip what the prediction names (mpc_lane.h, SUBSET 1).
double presolve_lambda_impl(const tpc_mpc_params* p) {
    if (p->horizon < 40 || p->max_iter < 2000 || p->smo_iters >= p->max_iter) return 0.0;
    const double t = (double)p->max_iter / 7.0;
    return t * t;
}

static double presolve_lambda(const tpc_mpc_params* p) { return presolve_lambda_impl(p); }

int presolve_begin(tpc_mpc_context* h, const tpc_mpc_params* p, int64_t n, const void* v, const void* dy, const void* dphi,
                   hipStream_t s, Presolve* ps) {
    *ps = Presolve();
    const int algo = pick_algo(h, compact_algo(p), 2, p->horizon, n, p->dtype, fma_usable(p));
    if (algo != TPC_MPC_ALGO_GROUP || !wants_cap_resolve(p, algo) || !h->collect_flags) return TPC_MPC_OK;
    const double lf = presolve_lambda(p);
    if (!(lf > 0.0) || h->pre_busy) return TPC_MPC_OK;
    // SIMDs of its own for the bit-exact kernel (mpc_lanex.h, SOLO), the rest for GROUP's persistent grid: 7 of 16 and 9 of
    // 16 -- the predicted set of the N = 40 stream is 20 % of a batch, eight instances per wavefront, and GROUP's pass is
    // bounded by its longest instance rather than by its share of the chip at the batch sizes it is AUTO's choice for
    // (16 384 x N = 40: 4.7 ms on the whole chip, 8.8 on 11 / 16).  A batch whose predicted set cannot run in ONE round of
    // those wavefronts is left to the second pass -- decided on the device, where the set's size is known; a batch too
    // large for a fifth of it to fit is not tried (presolve_share).
    if (!presolve_share(h, n, ps)) return TPC_MPC_OK;
    const int H = p->horizon;
    const int64_t out_b = pad256(n * 8), col_b = pad256(n * 4);
    Workspace ws;
    char* side = nullptr;
    int rc = presolve_scratch(h, H, p->dtype, n, 2 * out_b + col_b, &ws, &side);
    if (rc) return rc;
    char* b = side;
    const int64_t lane_b = 0;
    ps->side_front = b + lane_b;
    ps->side_rear = b + lane_b + out_b;
    ps->side_iters = (int32_t*)(b + lane_b + 2 * out_b);
    ps->queue = ws.order;
    ps->queue_len = ws.ticket + 1;
    ps->lambda_from = lf;
    CompactArgs a;
    compact_args(h, p, n, v, dy, dphi, ps->side_front, ps->side_rear, ps->side_iters, &a);
    HIP_TRY(h, hipEventRecord(h->pre_fork, s));
    HIP_TRY(h, hipStreamWaitEvent(h->pre_stream, h->pre_fork, 0));
    ps->on = true;   // (from here on presolve_finish must join the side stream, whatever happens)
    h->pre_busy = true;
    h->pre_group_waves = ps->group_waves;
    hipError_t e = hipErrorInvalidValue;
    switch (H) {
#define X(hh) case hh: e = lane_presolve_compact_h##hh(a, knobs_of(p), ws, lf, ps->limit, h->pre_stream); break;
        X(4) X(5) X(10) X(20) X(30) X(40)
#undef X
    }
    if (e != hipSuccess) return hip_fail(h, e, "kernel launch (presolve)");
    return TPC_MPC_OK;
}

int presolve_finish(tpc_mpc_context* h, const tpc_mpc_params* p, int64_t n, const void* v, const void* dy, const void* dphi,
                    void* front, void* rear, int32_t* iters, hipStream_t s, Presolve* ps) {
    if (ps->on) {
        ps->on = false;
        h->pre_busy = false;
        HIP_TRY(h, hipEventRecord(h->pre_done, h->pre_stream));
        HIP_TRY(h, hipStreamWaitEvent(s, h->pre_done, 0));
    }
    const int algo = pick_algo(h, compact_algo(p), 2, p->horizon, n, p->dtype, fma_usable(p));
    if (algo < 0 || !wants_cap_resolve(p, algo) || !h->collect_flags) return TPC_MPC_OK;
    int32_t* sel = iters ? iters : ps->select;
    if (ps->lambda_from > 0.0) {
        hipError_t e = presolve_merge(ps->queue, ps->queue_len, n, ps->side_front, ps->side_rear, ps->side_iters, front, rear, sel, ps->limit, s);
        if (e != hipSuccess) return hip_fail(h, e, "kernel launch (presolve merge)");
    }
    CompactArgs a;
    compact_args(h, p, n, v, dy, dphi, front, rear, sel, &a);
    Workspace ws2;
    int rc = resolve_workspace(h, p->horizon, p->dtype, n, &ws2);
    if (rc) return rc;
    hipError_t e = resolve_compact(p->horizon, a, knobs_of(p), ws2, s, ps->lambda_from, ps->queue_len, ps->limit);
    if (e != hipSuccess) return hip_fail(h, e, "kernel launch");
    return TPC_MPC_OK;
}

// Does mpc_queue_key_table.h speak about this solve?  Its counts were made with ONE parameter set, and an iteration count
// depends on every one of them: exact comparison against the header's constants, once per call; the kernel gets a flag.
// LANE_FMA only: GROUP at N = 20 runs the same coordinate-descent kernel, but is AUTO's choice for the small batches,
// which its persistent grid does not fill -- nothing measured says the order matters there, so it keeps lambda.
static bool queue_key_table_applies(const tpc_mpc_params* p, int algo) {
    return algo == TPC_MPC_ALGO_LANE_FMA && p->dtype == TPC_MPC_F64 && p->horizon == kQueueKeyH &&
           p->weight_y == kQueueKeyWeights[0] && p->weight_phi == kQueueKeyWeights[1] &&
           p->weight_steering_front == kQueueKeyWeights[2] && p->weight_steering_rear == kQueueKeyWeights[3] &&
           p->step_size == kQueueKeyStep && p->wheelbase == kQueueKeyWheelbase &&
           p->lower[0] == kQueueKeyLower && p->lower[1] == kQueueKeyLower &&
           p->upper[0] == kQueueKeyUpper && p->upper[1] == kQueueKeyUpper && p->eps == kQueueKeyEps &&
           p->max_iter == kQueueKeyMaxIter && p->smo_iters == kQueueKeySmoIters;
}

// the tolerance (or whatever pick_algo says) pass; with `ps`: AUTO's guarantee is the caller's business (presolve_finish),
// immediately unless ps->deferred
int compact_launch_ps(tpc_mpc_context* h, const tpc_mpc_params* p, int64_t n, const void* v, const void* dy,
                      const void* dphi, void* front, void* rear, int32_t* iters, hipStream_t s, Presolve* ps) {
    const int algo = pick_algo(h, compact_algo(p), 2, p->horizon, n, p->dtype, fma_usable(p));
    if (algo < 0) return fail(h, TPC_MPC_ERR_BAD_HORIZON, "the WAVE kernel exists for the specialised horizons with inputs*horizon <= 64 only; use LANE or AUTO");
    CompactArgs a;
    compact_args(h, p, n, v, dy, dphi, front, rear, iters, &a);
    a.work_hint = take_hint(h, n);
    a.table_key = h->opt_queue_key && queue_key_table_applies(p, algo) ? 1 : 0;
    h->last_queue_key = a.work_hint ? kQueueKeyHint : (a.table_key ? kQueueKeyTableUsed : kQueueKeyLambda);
    const bool fix = wants_cap_resolve(p, algo) && a.flags;
    int rc = TPC_MPC_OK;
    if (fix && !a.iters) rc = cap_iters_buffer(h, n, &a.iters);
    if (!rc && fix) rc = resolve_reserve(h, p->horizon, p->dtype, n);
    if (rc) return rc;
    ps->select = a.iters;
    Workspace ws;
    rc = prepare_workspace(h, algo, p->horizon, p->dtype, n, &ws);
    if (rc) return rc;
    hipError_t e = dispatch_compact(algo, p->horizon, p->dtype, a, knobs_of(p), ws, s);
    if (e != hipSuccess) return hip_fail(h, e, "kernel launch");
    if (ps->deferred) return TPC_MPC_OK;
    return presolve_finish(h, p, n, v, dy, dphi, front, rear, iters, s, ps);
}

int compact_launch(tpc_mpc_context* h, const tpc_mpc_params* p, int64_t n, const void* v, const void* dy,
                   const void* dphi, void* front, void* rear, int32_t* iters, hipStream_t s) {
    Presolve ps;
    int rc = presolve_begin(h, p, n, v, dy, dphi, s, &ps);
    if (!rc) rc = compact_launch_ps(h, p, n, v, dy, dphi, front, rear, iters, s, &ps);
    if (rc && ps.on) {   // the side stream got work: the caller's stream must not run ahead of it (scratch, outputs)
        h->pre_busy = false;
        (void)hipEventRecord(h->pre_done, h->pre_stream);
        (void)hipStreamWaitEvent(s, h->pre_done, 0);
    }
    return rc;
}

}  // namespace tpc

namespace {

// HOST arrays go through h->stage, and through these two functions alone.  stage_in gives every array of the table
// that is there a slot (tpc_mpc_stage.h: leading dimension stage_ld(n), 256-byte padded) and copies the inputs in;
// stage_out copies the outputs back and waits for them.  Row by row, n elements per row: a caller's ld > n (a shard of a
// wider batch) is neither over-read nor over-written.  On return of stage_in, t[c].dev is what the kernels take.
int stage_in(tpc_mpc_context* h, StagedArray* t, int count, int64_t n, hipStream_t s) {
    int rc = ensure(h, &h->stage, &h->stage_bytes, stage_layout(t, count, n));
    if (rc) return rc;
    for (int c = 0; c < count; ++c) {
        StagedArray& a = t[c];
        if (!a.ptr) continue;
        a.dev = (char*)h->stage + a.off;
        if (a.role & kStageIn)
            HIP_TRY(h, copy_rows(a.dev, stage_pitch(a, n) * a.width, a.ptr, a.ld * a.width, stage_elems(a, n) * a.width,
                                 a.rows, hipMemcpyHostToDevice, s));
    }
    return TPC_MPC_OK;
}
int stage_out(tpc_mpc_context* h, const StagedArray* t, int count, int64_t n, hipStream_t s) {
    for (int c = 0; c < count; ++c) {
        const StagedArray& a = t[c];
        if (a.ptr && (a.role & kStageOut))
            HIP_TRY(h, copy_rows(const_cast<void*>(a.ptr), a.ld * a.width, a.dev, stage_pitch(a, n) * a.width,
                                 stage_elems(a, n) * a.width, a.rows, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return TPC_MPC_OK;
}

// What only some users of staged_run need of their arrays in the caller's memory; each table is [NIn + NOut] and may
// be null
struct StagedExtra {
    const int64_t* ld = nullptr;      // leading dimension where not the call's (0: the call's)
    const int* width = nullptr;       // bytes per element where not 8 (0: 8)
    const int64_t* elems = nullptr;   // elements per row where not n (0: n): a row that is not per instance
    int inout = -1;                   // src[inout] is written too: its staged copy always goes back to it
};

// What the one-launch entries share after their argument checks: NIn input arrays (a null one is not staged) of rows[c]
// component rows and NOut output arrays of rows[NIn + c], n instances with the leading dimension ld in the caller's
// memory, run by `run(ld, in, out, s, host_flags)` -- on the calling thread for a host-only handle (host_flags !=
// null), else as a launch on s: on the caller's own DEVICE arrays and ld, or on the slots of HOST arrays (stage_in) and
// stage_ld(n).  On the stream: the gradient workspace grown to ws_bytes, the staging copies, the flag word zeroed, the
// launch, the copies back and a synchronise (HOST only), the stream order's event, the flags.
template <int NIn, int NOut, class Run>
int staged_run(tpc_mpc_context* h, int64_t n, int64_t ld, int mem, void* stream, uint32_t* flags_out, int64_t ws_bytes,
               const void* const (&src)[NIn], void* const (&dst)[NOut], const int64_t (&rows)[NIn + NOut], Run run,
               const StagedExtra& x = StagedExtra()) {
    if (h->host_only) {   // on the calling thread, straight from and into the caller's arrays
        uint32_t f = 0;
        (void)run(ld, src, dst, (hipStream_t) nullptr, &f);
        if (flags_out) *flags_out = f;
        return TPC_MPC_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    StreamOrderScope order(h, s);
    int rc = order.begin();
    if (rc) return rc;
    rc = ensure(h, &h->grad_ws, &h->grad_ws_bytes, pad256(ws_bytes));
    if (rc) return rc;
    const bool host = mem == TPC_MPC_HOST;
    StagedArray t[NIn + NOut];
    for (int c = 0; c < NIn + NOut; ++c)
        t[c] = staged(c < NIn ? src[c] : dst[c - NIn], c == x.inout ? kStageInOut : c < NIn ? kStageIn : kStageOut, rows[c],
                      x.ld && x.ld[c] ? x.ld[c] : ld, x.width && x.width[c] ? x.width[c] : 8, x.elems ? x.elems[c] : 0);
    if (host) {
        rc = stage_in(h, t, NIn + NOut, n, s);
        if (rc) return rc;
        ld = stage_ld(n);
    }
    const void* in[NIn];
    void* out[NOut];
    for (int c = 0; c < NIn; ++c) in[c] = t[c].dev;
    for (int c = 0; c < NOut; ++c) out[c] = t[NIn + c].dev;
    HIP_TRY(h, hipMemsetAsync(h->ws_words + 1, 0, sizeof(uint32_t), s));
    hipError_t e = run(ld, in, out, s, (uint32_t*)nullptr);
    if (e != hipSuccess) return hip_fail(h, e, "kernel launch");
    if (host) {
        rc = stage_out(h, t, NIn + NOut, n, s);
        if (rc) return rc;
    }
    rc = order.end();
    if (rc) return rc;
    return finish_flags(h, flags_out, s);
}

// the model's nine arrays, in[0..8] in the io's order, into the Args of a gradient, polish or tangent kernel
template <class Args> void bind_model(Args* a, const void* const* in) {
    a->A = (const double*)in[0]; a->B = (const double*)in[1]; a->C = (const double*)in[2];
    a->Q = (const double*)in[3]; a->R = (const double*)in[4]; a->lo = (const double*)in[5];
    a->hi = (const double*)in[6]; a->x0 = (const double*)in[7]; a->targets = (const double*)in[8];
}

// the ten tangent arrays of a tpc_mpc_tangents in Dirs' order, from in[0..9]
tangent::Dirs bind_dirs(const void* const* in) {
    tangent::Dirs d;
    d.tA = (const double*)in[0]; d.tB = (const double*)in[1]; d.tC = (const double*)in[2];
    d.tQ = (const double*)in[3]; d.tR = (const double*)in[4]; d.tlo = (const double*)in[5];
    d.thi = (const double*)in[6]; d.tx0 = (const double*)in[7]; d.ttargets = (const double*)in[8];
    d.tnlt = (const double*)in[9];
    return d;
}

// The per-step arrays of the closed loops (rollout_impl, rollout_newton_impl) as a staging table: new_last_targets and
// the plant's disturbance in, seven outputs; a null one is not there.  The kernels take t[c].dev with the leading
// dimensions below: the caller's DEVICE arrays as they are, or after stage_steps the slots of HOST arrays, which
// stage_out(h, g.t, kStepCount, n, s) copies back.
enum { kStepNlt, kStepDist, kStepCtrl, kStepStates, kStepIters, kStepSeq, kStepStatus, kStepRin, kStepRout, kStepCount };
struct StepArrays {
    StagedArray t[kStepCount];
    int64_t ld_nlt, ld_d, ld_out;
    template <class T = void> T* at(int c) const { return (T*)t[c].dev; }
};
// the caller's arrays; es: bytes per element of the loop's arithmetic (iters and status are int32, the residuals fp64
// whatever it is); q null: a loop without the polish's outputs
StepArrays step_arrays(const tpc_mpc_general_io* io, int H, int64_t S, int es, const void* new_last_targets,
                       const tpc_mpc_plant* plant, void* controls_out, void* states_out, int32_t* iters_out,
                       void* sequences_out, const tpc_mpc_polish* q) {
    const int64_t I = io->inputs, ld = io->ld;
    const void* dist = plant ? plant->disturbance : nullptr;
    StepArrays g;
    g.ld_nlt = g.ld_out = ld;
    g.ld_d = dist ? plant->ld_d : 0;
    g.t[kStepNlt] = staged(new_last_targets, kStageIn, 2 * S, ld, es);
    g.t[kStepDist] = staged(dist, kStageIn, 2 * S, g.ld_d, es);
    g.t[kStepCtrl] = staged(controls_out, kStageOut, S * I, ld, es);
    g.t[kStepStates] = staged(states_out, kStageOut, 2 * S, ld, es);
    g.t[kStepIters] = staged(iters_out, kStageOut, S, ld, 4);
    g.t[kStepSeq] = staged(sequences_out, kStageOut, S * H * I, ld, es);
    g.t[kStepStatus] = staged(q ? q->status : nullptr, kStageOut, S, ld, 4);
    g.t[kStepRin] = staged(q ? q->residual_in : nullptr, kStageOut, S, ld, 8);
    g.t[kStepRout] = staged(q ? q->residual_out : nullptr, kStageOut, S, ld, 8);
    return g;
}
// HOST arrays only: the slots' leading dimensions, and with stage_steps the slots and the inputs copied in
void staged_step_lds(StepArrays* g, int64_t n) {
    g->ld_nlt = g->ld_out = stage_ld(n);
    if (g->t[kStepDist].ptr) g->ld_d = stage_ld(n);
}
int stage_steps(tpc_mpc_context* h, StepArrays* g, int64_t n, hipStream_t s) {
    staged_step_lds(g, n);
    return stage_in(h, g->t, kStepCount, n, s);
}

// ---- The two phases of the Newton-first entries, once ----
// tpc_mpc_rollout_newton / _plant, tpc_mpc_solve_batch_compact_exact (_rows, _from) and tpc_mpc_rollout_compact_exact
// are this frame around what is their own.  Phase 1 is ONE launch that verifies most instances.  With
// TPC_MPC_NEWTON_FALLBACK_SOLVE its lanes queue the instances they could not verify (mpc_newton_fallback.h); one 4-byte
// read-back of the queue's length and a synchronise -- the only ones, and only in that mode -- sit between the phases.
// The queued instances are gathered into a compact batch (h->newton_fb, leading dimension ldc: the count rounded up to
// a wavefront), run through the general path and scattered back.  What holds the two together, for every entry:
//   - h->newton is the entry's own working set (ws_bytes), then the queue ([stage_ld(n)] int32) and two words: [0] the
//     queue's length, [1] phase 1's flags.  Phase 1 gets the queue only with FALLBACK_SOLVE: fb_index is null otherwise,
//     nothing is queued and "not polished" is raised instead (raised_flags).
//   - every general entry the fallback calls resets the handle's flag word (h->ws_words + 1).  So phase 1 raises its
//     flags in word [1], and they are merged into the handle's word after the fallback -- or after that word is zeroed,
//     when nothing fell back.
//   - the fallback calls those entries with TPC_MPC_DEVICE and no flags_out: no staging, no synchronise.  So nothing
//     writes h->stage between phase 1 and the copies back, and the HOST arrays staged there (t) outlive the fallback.
// A host-only handle never gets here: the entries run phase 1 on the calling thread before anything touches HIP.
struct NewtonPhase {
    char* ws;             // h->newton: ws_bytes of the entry's own
    int32_t* fb_index;    // the queue (in no particular order); null without FALLBACK_SOLVE
    uint32_t* fb_count;   // word [0]
    uint32_t* flags;      // word [1]
    hipStream_t s;
    bool staged;          // HOST arrays: t[c].dev are slots with the leading dimension stage_ld(n)
};
inline int newton_nothing(const NewtonPhase&) { return TPC_MPC_OK; }
// grad_bytes: what h->grad_ws must hold (0: not grown).  t[count]: the call's arrays, staged when mem is HOST.
// On the stream, in this order: fill(f) -- the entry's own working set; the words zeroed; the staging copies;
// phase1(f), the launch; [the read-back]; fallback(f, count, ldc), or the handle's flag word zeroed; the flag merge;
// back(f) -- copies back that are no staged arrays; the staged copies back and their synchronise; the stream order's
// event; the flags.
template <class Fill, class Phase1, class Fallback, class Back>
int newton_two_phase(tpc_mpc_context* h, int64_t n, bool solve, int mem, void* stream, uint32_t* flags_out,
                     int64_t ws_bytes, int64_t grad_bytes, StagedArray* t, int count, Fill fill, Phase1 phase1,
                     Fallback fallback, Back back) {
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    StreamOrderScope order(h, s);
    int rc = order.begin();
    if (rc) return rc;
    const bool host = mem == TPC_MPC_HOST;
    const int64_t o_words = ws_bytes + stage_ld(n) * 4;
    rc = ensure(h, &h->newton, &h->newton_bytes, o_words + 256);
    if (!rc && grad_bytes > 0) rc = ensure(h, &h->grad_ws, &h->grad_ws_bytes, pad256(grad_bytes));
    if (rc) return rc;
    char* w = (char*)h->newton;
    uint32_t* d_words = (uint32_t*)(w + o_words);
    const NewtonPhase f{w, solve ? (int32_t*)(w + ws_bytes) : nullptr, d_words, d_words + 1, s, host};
    rc = fill(f);
    if (rc) return rc;
    HIP_TRY(h, hipMemsetAsync(d_words, 0, 8, s));
    if (host) {
        rc = stage_in(h, t, count, n, s);
        if (rc) return rc;
    }
    hipError_t e = phase1(f);
    if (e != hipSuccess) return hip_fail(h, e, "kernel launch");

    uint32_t queued = 0;
    if (solve) {
        HIP_TRY(h, hipMemcpyAsync(&queued, d_words, sizeof(queued), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    if (queued > 0) {
        rc = fallback(f, (int64_t)queued, stage_ld(queued));
        if (rc) return rc;
    } else {
        HIP_TRY(h, hipMemsetAsync(h->ws_words + 1, 0, sizeof(uint32_t), s));
    }
    e = rollout_newton_merge_flags(h->ws_words + 1, f.flags, s);
    if (e != hipSuccess) return hip_fail(h, e, "flag merge launch");

    rc = back(f);
    if (!rc && host) rc = stage_out(h, t, count, n, s);
    if (!rc) rc = order.end();
    if (rc) return rc;
    return finish_flags(h, flags_out, s);
}

// Rows of the compact batch in h->newton_fb, leading dimension ldc: fp64 rows first, in the order taken, the int32 rows
// (iters, status) behind them.  take() before reserve(), at() / at32() after.
struct FallbackRows {
    int64_t ldc, total = 0;
    char* fb = nullptr;
    explicit FallbackRows(int64_t ld) : ldc(ld) {}
    // an array of `rows` fp64 rows: its first row, or -1 when it is not there (it then takes none)
    int64_t take(bool there, int64_t rows) { const int64_t at = total; if (there) total += rows; return there ? at : -1; }
    // grows h->newton_fb to the fp64 rows taken and rows32 int32 rows
    int reserve(tpc_mpc_context* h, int64_t rows32) {
        const int rc = ensure(h, &h->newton_fb, &h->newton_fb_bytes, total * ldc * 8 + rows32 * ldc * 4);
        fb = (char*)h->newton_fb;
        return rc;
    }
    double* at(int64_t row) const { return row < 0 ? nullptr : (double*)(fb + row * ldc * 8); }
    int32_t* at32(bool there, int64_t row32) const { return there ? (int32_t*)(fb + total * ldc * 8 + row32 * ldc * 4) : nullptr; }
};

// The general form of `count` queued instances from the batch's rows: the nine model arrays at row[0..8], the io's order
tpc_mpc_general_io fallback_io(const FallbackRows& L, int I, int64_t count, const int64_t* row) {
    tpc_mpc_general_io io{};
    io.inputs = I; io.n = count; io.ld = L.ldc;
    io.A = L.at(row[0]); io.B = L.at(row[1]); io.C = L.at(row[2]); io.Q = L.at(row[3]); io.R = L.at(row[4]);
    io.lower = L.at(row[5]); io.upper = L.at(row[6]); io.x0 = L.at(row[7]); io.targets = L.at(row[8]);
    return io;
}
// ... of the compact entries (I = 2): the 20 + 2H model rows from `first` on, as the gather-expand kernels' batch and
// as the io
constexpr int64_t compact_model_rows(int H) { return 20 + 2 * (int64_t)H; }
tpc_mpc_general_io fallback_compact_model(const FallbackRows& L, int64_t first, int H, int64_t count,
                                          const int32_t* index, FallbackBatch* b) {
    const int64_t comps[9] = {4, 4, 2, 2, 2, 2, 2, 2, 2 * (int64_t)H};
    int64_t row[9];
    for (int c = 0; c < 9; ++c) { row[c] = first; first += comps[c]; }
    const tpc_mpc_general_io io = fallback_io(L, 2, count, row);
    b->count = count; b->ld = L.ldc; b->index = index; b->H = H;
    b->A = (double*)io.A; b->B = (double*)io.B; b->C = (double*)io.C; b->Q = (double*)io.Q; b->R = (double*)io.R;
    b->lo = (double*)io.lower; b->hi = (double*)io.upper; b->x0 = (double*)io.x0; b->targets = (double*)io.targets;
    return io;
}

// The per-step outputs of a polished loop (null: not asked for): the caller's, or their rows in the compact batch
struct StepOutputs {
    void *ctrl, *states, *seq, *rin, *rout;
    int32_t *iters, *status;
};
// their rows in the compact batch, taken for those of `d` that are there (controls always are) ...
struct StepRows { int64_t ctrl, states, seq, rin, rout; };
StepRows take_step_rows(FallbackRows* L, const StepOutputs& d, int I, int H, int64_t S) {
    const int64_t ctrl = L->take(true, S * I), states = L->take(d.states, S * 2), seq = L->take(d.seq, S * H * I);
    return StepRows{ctrl, states, seq, L->take(d.rin, S), L->take(d.rout, S)};
}
// ... as pointers, once the batch is reserved; the int32 rows: iters (`with_iters`: S rows, there or not), then status
StepOutputs step_outputs_at(const FallbackRows& L, const StepRows& r, const StepOutputs& d, int64_t S, bool with_iters) {
    return StepOutputs{L.at(r.ctrl), L.at(r.states), L.at(r.seq), L.at(r.rin), L.at(r.rout),
                       L.at32(with_iters && d.iters, 0), L.at32(d.status, with_iters ? S : 0)};
}
// ... and the table that scatters them from the compact batch (f, ldc) to the caller's (d, ld_out)
NewtonMove step_scatter(int64_t count, const int32_t* index, const StepOutputs& f, const StepOutputs& d, int I, int H,
                        int64_t S, int64_t ldc, int64_t ld_out) {
    NewtonMove sc{count, index, 0, {}};
    auto add = [&](const void* src, void* dst, int64_t rows, int bytes) {
        if (dst) sc.set[sc.sets++] = NewtonRows{src, dst, rows, ldc, ld_out, bytes};
    };
    add(f.ctrl, d.ctrl, S * I, 8); add(f.states, d.states, S * 2, 8); add(f.seq, d.seq, S * H * I, 8);
    add(f.rin, d.rin, S, 8); add(f.rout, d.rout, S, 8); add(f.iters, d.iters, S, 4); add(f.status, d.status, S, 4);
    return sc;
}

// tpc_mpc_solve_batch_compact's arrays as a staging table: v, dy, dphi in, front and rear out in the solve's
// arithmetic, the optional iteration counts (int32) out
enum { kCompactArrays = 6 };
void compact_table(StagedArray (&t)[kCompactArrays], int dtype, int64_t n, const void* v, const void* dy, const void* dphi,
                   void* front, void* rear, int32_t* iters) {
    const int es = (int)esize(dtype);
    t[0] = staged(v, kStageIn, 1, n, es);
    t[1] = staged(dy, kStageIn, 1, n, es);
    t[2] = staged(dphi, kStageIn, 1, n, es);
    t[3] = staged(front, kStageOut, 1, n, es);
    t[4] = staged(rear, kStageOut, 1, n, es);
    t[5] = staged(iters, kStageOut, 1, n, 4);
}
// the bytes of h->stage that a HOST call of it takes at most (iters asked for): what tpc_mpc_reserve grows h->stage to
int64_t compact_stage_bytes(int dtype, int64_t n) {
    static int32_t there;   // any array: the layout asks only whether one is there
    StagedArray t[kCompactArrays];
    compact_table(t, dtype, n, &there, &there, &there, &there, &there, &there);
    return stage_layout(t, kCompactArrays, n);
}

}  // namespace

extern "C" {

int tpc_mpc_abi_version(void) { return TPC_MPC_ABI_VERSION; }

int tpc_mpc_supported_horizons(int* out, int cap) {
    const int n = (int)(sizeof(kHorizons) / sizeof(kHorizons[0]));
    for (int i = 0; i < n && i < cap && out; ++i) out[i] = kHorizons[i];
    return n;
}

const char* tpc_mpc_build_info(void) {
    // assembled once from what each LANE translation unit recorded about its own build (csrc/Makefile);
    // static storage: valid for the process lifetime, as the header promises
    static char info[512];
    static std::once_flag once;
    std::call_once(once, [] {
        std::snprintf(info, sizeof(info),
                      "libtpc_mpc abi %d gfx950; lane units: h4[%s] h5[%s] h10[%s] h20[%s] h30[%s] h40[%s]",
                      TPC_MPC_ABI_VERSION, lane_build_h4(), lane_build_h5(), lane_build_h10(), lane_build_h20(),
                      lane_build_h30(), lane_build_h40());
    });
    return info;
}

int tpc_mpc_default_params(tpc_mpc_params* p, int horizon) {
    if (!p) return TPC_MPC_ERR_BAD_ARG;
    std::memset(p, 0, sizeof(*p));
    p->horizon = horizon;
    p->dtype = TPC_MPC_F64;
    p->algo = TPC_MPC_ALGO_AUTO;
    p->eps = 0.01;            // mpc.h:104
    p->max_iter = 10000;      // mpc.h:103
    p->smo_iters = 50;        // mpc.h:319
    p->step_size = 0.1;       // src/trajectory_point_follower.cpp:96
    p->wheelbase = 0.21;      // include/trajectory_point_follower.h:47
    p->weight_y = 20;         // src/trajectory_point_follower.cpp:92-95
    p->weight_phi = 7;
    p->weight_steering_front = 0.0005;
    p->weight_steering_rear = 10;
    const double alpha_max = 22 * M_PI / 180;   // src/trajectory_point_follower.cpp:16-18
    p->lower[0] = p->lower[1] = -alpha_max;
    p->upper[0] = p->upper[1] = alpha_max;
    return horizon_ok(horizon) ? TPC_MPC_OK : TPC_MPC_ERR_BAD_HORIZON;
}

int tpc_mpc_create(int device, tpc_mpc_handle* out) {
    return guarded(nullptr, [&]() -> int {
        if (!out) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null out pointer");
        *out = nullptr;
        if (device == TPC_MPC_DEVICE_NONE) {   // host-only: no HIP call, here or ever
            tpc_mpc_context* h = new (std::nothrow) tpc_mpc_context;
            if (!h) return fail(nullptr, TPC_MPC_ERR_ALLOC, "out of host memory");
            h->device = -1;
            h->host_only = true;
            *out = h;
            return TPC_MPC_OK;
        }
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0)
            return fail(nullptr, TPC_MPC_ERR_NO_DEVICE, "no HIP device: %s",
                        e != hipSuccess ? hipGetErrorString(e) : "count == 0");
        if (device < 0 || device >= count) return fail(nullptr, TPC_MPC_ERR_NO_DEVICE, "device index out of range");
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, device);
        if (e != hipSuccess) return fail(nullptr, TPC_MPC_ERR_NO_DEVICE, "%s", hipGetErrorString(e));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(nullptr, TPC_MPC_ERR_NO_DEVICE, "device is %s, this library carries gfx950 code only",
                        prop.gcnArchName);
        return context_new(device, prop.multiProcessorCount, out);
    });
}

int tpc_mpc_destroy(tpc_mpc_handle h) {
    if (!h) return TPC_MPC_OK;
    return guarded(nullptr, [&]() -> int {
        if (h->host_only) { delete h; return TPC_MPC_OK; }
        (void)hipSetDevice(h->device);
        one_shot_destroy(h);   // stops the resident kernel before its mailbox goes away
        comm_destroy(h);
        for (int i = 0; i < tpc_mpc_context::kMaxKids; ++i) {
            if (h->kid_stream[i]) { (void)hipStreamSynchronize(h->kid_stream[i]); (void)hipStreamDestroy(h->kid_stream[i]); }
            if (h->kid_done[i]) (void)hipEventDestroy(h->kid_done[i]);
            if (h->kids[i]) (void)tpc_mpc_destroy(h->kids[i]);
        }
        if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
        if (h->ws_state) (void)hipFree(h->ws_state);
        if (h->ws_words) (void)hipFree(h->ws_words);
        if (h->stage) (void)hipFree(h->stage);
        if (h->roll) (void)hipFree(h->roll);
        if (h->cap_iters) (void)hipFree(h->cap_iters);
        if (h->grad_ws) (void)hipFree(h->grad_ws);
        if (h->newton) (void)hipFree(h->newton);
        if (h->newton_fb) (void)hipFree(h->newton_fb);
        if (h->mix) (void)hipFree(h->mix);
        if (h->gather) (void)hipFree(h->gather);
        if (h->pre_stream) { (void)hipStreamSynchronize(h->pre_stream); (void)hipStreamDestroy(h->pre_stream); }
        if (h->pre_fork) (void)hipEventDestroy(h->pre_fork);
        if (h->pre_done) (void)hipEventDestroy(h->pre_done);
        if (h->pre) (void)hipFree(h->pre);
        if (h->hint_own) (void)hipFree(h->hint_own);
        if (h->pin_host) (void)hipHostFree(h->pin_host);
        if (h->done_ev) (void)hipEventDestroy(h->done_ev);
        for (auto& e : h->ev) if (e) (void)hipEventDestroy(e);
        delete h;
        return TPC_MPC_OK;
    });
}

const char* tpc_mpc_last_error(tpc_mpc_handle h) { return h ? h->err : g_create_error; }

int tpc_mpc_solve_batch_compact(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                const void* delta_y, const void* delta_phi, void* steering_front,
                                void* steering_rear, int32_t* iters, uint32_t* flags_out, int mem,
                                void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p);
        if (rc) return rc;
        rc = check_compact_model(h, p);
        if (rc) return rc;
        rc = check_batch(h, n, mem);
        if (rc) return rc;
        if (n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        if (!v || !delta_y || !delta_phi || !steering_front || !steering_rear)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        StreamOrderScope order(h, s);
        rc = order.begin();
        if (rc) return rc;
        HIP_TRY(h, hipMemsetAsync(h->ws_words + 1, 0, sizeof(uint32_t), s));
        const bool host = mem == TPC_MPC_HOST;
        StagedArray t[kCompactArrays];
        compact_table(t, p->dtype, n, v, delta_y, delta_phi, steering_front, steering_rear, iters);
        if (host) {
            rc = stage_in(h, t, kCompactArrays, n, s);
            if (rc) return rc;
        }
        rc = compact_launch(h, p, n, t[0].dev, t[1].dev, t[2].dev, t[3].dev, t[4].dev, (int32_t*)t[5].dev, s);
        if (rc) return rc;
        if (host) {
            rc = stage_out(h, t, kCompactArrays, n, s);
            if (rc) return rc;
        }
        rc = order.end();
        if (rc) return rc;
        return finish_flags(h, flags_out, s);
    });
}

int tpc_mpc_solve_one(tpc_mpc_handle h, const tpc_mpc_params* p, double v, double delta_y,
                      double delta_phi, double* steering_front, double* steering_rear) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (!steering_front || !steering_rear) return fail(h, TPC_MPC_ERR_BAD_ARG, "null output pointer");
        int rc = check_common(h, p, true);
        if (rc) return rc;
        rc = check_compact_model(h, p);
        if (rc) return rc;
        // the host path (csrc/tpc_mpc_host.cpp): a host-only handle always, a GPU handle up to the horizon its option names
        if (h->host_only || p->horizon <= h->opt_host_horizon) {
            // (a host-only handle has no bit-exact kernels to send a tie-prone AUTO request to: include/tpc_mpc.h says so)
            const int want = h->host_only ? p->algo : compact_algo(p);
            const bool takes = p->dtype == TPC_MPC_F64 && (want == TPC_MPC_ALGO_AUTO || want == TPC_MPC_ALGO_LANE_FMA) &&
                               fma_usable(p) && horizon_specialised(p->horizon) && host_path_usable();
            if (takes) {
                int iters = 0;
                unsigned flags = 0;
                if (host_solve_one(p, v, delta_y, delta_phi, steering_front, steering_rear, &iters, &flags) == 0) {
                    h->one_flags = flags;
                    h->one_iters = iters;
                    h->one_valid = true;
                    // AUTO's guarantee for a solve that ended on the cap: dlib's bits need the bit-exact LANE kernels
                    if ((flags & TPC_MPC_FLAG_MAX_ITER) && !h->host_only && p->algo == TPC_MPC_ALGO_AUTO && p->max_iter > 0 &&
                        (p->options & TPC_MPC_PARAM_FAST_CAPPED) == 0) {
                        tpc_mpc_params q = *p;
                        q.algo = TPC_MPC_ALGO_LANE;
                        return one_shot_solve(h, &q, v, delta_y, delta_phi, steering_front, steering_rear);
                    }
                    return TPC_MPC_OK;
                }
            }
            if (h->host_only)
                return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle: the host path takes fp64, AUTO or LANE_FMA, horizons 4 5 10 20 30 40, "
                                                      "finite bounds with upper > lower, on a CPU with fused multiply-add");
        }
        // (no HIP call on the resident path: the parts of one_shot_solve that launch or wait select the device themselves)
        return one_shot_solve(h, p, v, delta_y, delta_phi, steering_front, steering_rear);
    });
}

int tpc_mpc_last_flags(tpc_mpc_handle h, uint32_t* flags, int32_t* iters) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (!h->one_valid) return fail(h, TPC_MPC_ERR_BAD_ARG, "no tpc_mpc_solve_one on this handle yet");
        if (flags) *flags = h->one_flags;
        if (iters) *iters = h->one_iters;
        return TPC_MPC_OK;
    });
}

int tpc_mpc_solve_batch_general(tpc_mpc_handle h, const tpc_mpc_params* p,
                                const tpc_mpc_general_io* io, uint32_t* flags_out, int mem,
                                void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p);
        if (rc) return rc;
        rc = check_general_io(h, io, mem);
        if (rc) return rc;
        if (io->n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        rc = check_model(h, io, io->u0 != nullptr);
        if (rc) return rc;
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        const int64_t es = (int64_t)esize(p->dtype);
        const int I = io->inputs, H = p->horizon;
        const int64_t n = io->n;
        const int algo = pick_algo(h, p->algo, I, H, n, p->dtype, fma_general_usable(H, io->controls_inout, io->v_inout), false,
                                   group_general_usable(p->dtype, H, io->controls_inout, io->v_inout));
        if (algo < 0) return fail(h, TPC_MPC_ERR_BAD_HORIZON, "the WAVE kernel exists for the specialised horizons with inputs*horizon <= 64 only; use LANE or AUTO");
        StreamOrderScope order(h, s);
        rc = order.begin();
        if (rc) return rc;

        GeneralArgs a;
        std::memset(&a, 0, sizeof(a));
        a.n = n;
        a.shift_controls = 1;
        // HOST arrays: component c of the caller's array starts at base + c*ld and only its first n
        // elements belong to this call (a shard passes base + k0 and the full batch's ld), so every
        // component row is copied on its own -- n elements, never ld -- into a staging array whose
        // leading dimension is n rounded up to a wavefront.
        const int64_t lds = (n + 63) / 64 * 64;
        const int comps[12] = {4, 2 * I, 2, 2, I, I, I, 2, 2 * H, H * I, H * I, I};
        int64_t off[13] = {0};
        char* b = nullptr;
        if (mem == TPC_MPC_DEVICE) {
            a.ld = io->ld;
            a.A = io->A; a.B = io->B; a.C = io->C; a.Q = io->Q; a.R = io->R; a.lo = io->lower; a.hi = io->upper;
            a.x0 = io->x0; a.targets = io->targets; a.controls = io->controls_inout; a.v = io->v_inout;
            a.u0 = io->u0; a.iters = io->iters;
        } else {
            const void* src[12] = {io->A, io->B, io->C, io->Q, io->R, io->lower, io->upper, io->x0, io->targets,
                                   io->controls_inout, io->v_inout, nullptr};
            int64_t total = 0;
            for (int c = 0; c < 12; ++c) { off[c] = total; total += pad256((int64_t)comps[c] * lds * es); }
            off[12] = total;
            total += pad256(n * 4);
            rc = ensure(h, &h->stage, &h->stage_bytes, total);
            if (rc) return rc;
            b = (char*)h->stage;
            for (int c = 0; c < 11; ++c)
                if (src[c])
                    HIP_TRY(h, copy_rows(b + off[c], lds * es, src[c], io->ld * es, n * es, comps[c],
                                         hipMemcpyHostToDevice, s));
            a.ld = lds;
            a.A = b + off[0]; a.B = b + off[1]; a.C = b + off[2]; a.Q = b + off[3]; a.R = b + off[4];
            a.lo = b + off[5]; a.hi = b + off[6]; a.x0 = b + off[7]; a.targets = b + off[8];
            a.controls = io->controls_inout ? b + off[9] : nullptr;
            a.v = io->v_inout ? b + off[10] : nullptr;
            a.u0 = b + off[11];
            a.iters = io->iters ? (int32_t*)(b + off[12]) : nullptr;
        }
        a.flags = h->ws_words + 1;
        a.work_hint = take_hint(h, n);
        const bool fix = wants_cap_resolve(p, algo) && !a.controls && !a.v;
        if (fix && !a.iters) {
            rc = cap_iters_buffer(h, n, &a.iters);
            if (rc) return rc;
        }
        if (fix) {
            rc = resolve_reserve(h, H, p->dtype, n);
            if (rc) return rc;
        }

        Workspace ws;
        rc = prepare_workspace(h, algo, H, p->dtype, n, &ws, 1);
        if (rc) return rc;
        HIP_TRY(h, hipMemsetAsync(h->ws_words + 1, 0, sizeof(uint32_t), s));
        hipError_t e = dispatch_general(algo, I, H, p->dtype, a, knobs_of(p), ws, s);
        if (e == hipSuccess && fix) {
            Workspace ws2;
            rc = resolve_workspace(h, H, p->dtype, n, &ws2);
            if (rc) return rc;
            e = resolve_general(I, H, a, knobs_of(p), ws2, s);
        }
        if (e != hipSuccess) return hip_fail(h, e, "kernel launch");
        if (mem == TPC_MPC_HOST) {
            const int64_t hp = io->ld * es, dp = lds * es, w = n * es;
            HIP_TRY(h, copy_rows(io->u0, hp, a.u0, dp, w, I, hipMemcpyDeviceToHost, s));
            if (io->controls_inout)
                HIP_TRY(h, copy_rows(io->controls_inout, hp, a.controls, dp, w, H * I, hipMemcpyDeviceToHost, s));
            if (io->v_inout) HIP_TRY(h, copy_rows(io->v_inout, hp, a.v, dp, w, H * I, hipMemcpyDeviceToHost, s));
            if (io->iters) HIP_TRY(h, hipMemcpyAsync(io->iters, a.iters, n * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(h, hipStreamSynchronize(s));
        }
        rc = order.end();
        if (rc) return rc;
        return finish_flags(h, flags_out, s);
    });
}

int tpc_mpc_solve_batch_general_backward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                         const tpc_mpc_general_grad* g, uint32_t* flags_out, int mem, void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_solve_batch_general_backward");
        rc = check_general_io(h, io, mem);
        if (rc) return rc;
        if (!g) return fail(h, TPC_MPC_ERR_BAD_ARG, "null gradient struct");
        rc = check_host_only_pass(h, mem, "backward pass");
        if (rc) return rc;
        if (io->n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        rc = check_model(h, io);
        if (rc) return rc;
        if (!g->controls || !g->grad_controls) return fail(h, TPC_MPC_ERR_BAD_ARG, "null controls / grad_controls");
        const int I = io->inputs, H = p->horizon;
        const int64_t n = io->n;
        // the io's and g's arrays in order: 11 inputs, then 10 outputs, with their component counts
        const void* src[11] = {io->A, io->B, io->C, io->Q, io->R, io->lower, io->upper, io->x0, io->targets,
                               g->controls, g->grad_controls};
        void* dst[10] = {g->dA, g->dB, g->dC, g->dQ, g->dR, g->dlower, g->dupper, g->dx0, g->dtargets, g->kkt_residual};
        const int64_t rows[21] = {4, 2 * I, 2, 2, I, I, I, 2, 2 * H, H * I, H * I,
                                  4, 2 * I, 2, 2, I, I, I, 2, 2 * H, 1};
        return staged_run(h, n, io->ld, mem, stream, flags_out, grad_scratch_bytes(I, H, n), src, dst, rows,
                          [&](int64_t ld, const void* const* in, void* const* out, hipStream_t s, uint32_t* hf) {
                              grad::Args a;
                              std::memset(&a, 0, sizeof(a));
                              a.n = n; a.ld = ld;
                              bind_model(&a, in);
                              a.u = (const double*)in[9]; a.g = (const double*)in[10];
                              a.dA = (double*)out[0]; a.dB = (double*)out[1]; a.dC = (double*)out[2];
                              a.dQ = (double*)out[3]; a.dR = (double*)out[4]; a.dlo = (double*)out[5];
                              a.dhi = (double*)out[6]; a.dx0 = (double*)out[7]; a.dtargets = (double*)out[8];
                              a.kkt = (double*)out[9];
                              if (hf) { *hf = grad_general_host(I, H, a); return hipSuccess; }
                              return grad_general(I, H, a, h->grad_ws, h->ws_words + 1, s);
                          });
    });
}

int tpc_mpc_polish_batch_general(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                 const tpc_mpc_polish* q, uint32_t* flags_out, int mem, void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_polish_batch_general");
        rc = check_general_io(h, io, mem);
        if (rc) return rc;
        rc = check_polish(h, q);
        if (rc) return rc;
        rc = check_host_only_pass(h, mem, "polish");
        if (rc) return rc;
        if (io->n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        rc = check_model(h, io);
        if (rc) return rc;
        if (!io->controls_inout) return fail(h, TPC_MPC_ERR_BAD_ARG, "null controls_inout: the sequence to polish");
        const int I = io->inputs, H = p->horizon;
        const int64_t n = io->n;
        // the arrays in order: 10 inputs (controls_inout is polished in place: in and out), then u0, the residuals
        // (fp64) and the status (int32), with their component counts
        const void* src[10] = {io->A, io->B, io->C, io->Q, io->R, io->lower, io->upper, io->x0, io->targets,
                               io->controls_inout};
        void* dst[4] = {io->u0, q->residual_in, q->residual_out, q->status};
        const int64_t rows[14] = {4, 2 * I, 2, 2, I, I, I, 2, 2 * H, H * I, I, 1, 1, 1};
        int width[14] = {0};
        width[13] = 4;
        StagedExtra x;
        x.width = width;
        x.inout = 9;
        return staged_run(h, n, io->ld, mem, stream, flags_out, polish_scratch_bytes(I, H, n), src, dst, rows,
                          [&](int64_t ld, const void* const* in, void* const* out, hipStream_t s, uint32_t* hf) {
                              polish::Args a;
                              std::memset(&a, 0, sizeof(a));
                              a.n = n; a.ld = ld; a.tol = q->tol; a.max_rounds = q->max_rounds;
                              bind_model(&a, in);
                              a.u = (double*)in[9];
                              a.u0 = (double*)out[0]; a.res_in = (double*)out[1]; a.res_out = (double*)out[2];
                              a.status = (int32_t*)out[3];
                              if (hf) { *hf = polish_general_host(I, H, a); return hipSuccess; }
                              return polish_general(I, H, a, h->grad_ws, h->ws_words + 1, s);
                          },
                          x);
    });
}

namespace {

// tpc_mpc_rollout, tpc_mpc_rollout_record (record: sequences_out is required) and tpc_mpc_rollout_polished (polished:
// q is required, every step's solve is followed by the fused polish + step kernel instead of the step kernel)
int rollout_impl(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, int32_t steps,
                 const void* new_last_targets, void* controls_out, void* states_out, int32_t* iters_out,
                 void* sequences_out, bool record, bool polished, const tpc_mpc_polish* q, uint32_t* flags_out, int mem,
                 void* stream, const tpc_mpc_plant* plant = nullptr) {
    return guarded(h, [&]() -> int {
        // the polished loop checks its arguments before it asks for the device, so that a host-only handle reports them
        // (plant: tpc_mpc_rollout_plant, which has checked the plant itself; null: the controller's model moves the state)
        int rc = check_common(h, p, polished || plant);
        if (rc) return rc;
        if (polished && p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_rollout_polished");
        rc = check_general_io(h, io, mem);
        if (rc) return rc;
        if (polished) rc = check_polish(h, q);
        if (!rc) rc = check_steps(h, steps);
        if (rc) return rc;
        if (h->host_only)
            return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle (TPC_MPC_DEVICE_NONE): the closed loops run on the device only");
        if (io->n == 0 || steps == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        rc = check_model(h, io, controls_out != nullptr);
        if (rc) return rc;
        if (record && !sequences_out) return fail(h, TPC_MPC_ERR_BAD_ARG, "null sequences_out");
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        const int64_t es = (int64_t)esize(p->dtype);
        const int I = io->inputs, H = p->horizon;
        const int64_t n = io->n, ld = io->ld;
        const int algo = pick_algo(h, p->algo, I, H, n, p->dtype, false, false, group_general_usable(p->dtype, H, (const void*)1, (const void*)1));
        if (algo < 0) return fail(h, TPC_MPC_ERR_BAD_HORIZON, "the WAVE kernel exists for the specialised horizons with inputs*horizon <= 64 only; use LANE or AUTO");
        StreamOrderScope order(h, s);
        rc = order.begin();
        if (rc) return rc;
        const bool host = mem == TPC_MPC_HOST;
        const hipMemcpyKind in_kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        const hipMemcpyKind out_kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;

        // The handle's working set, leading dimension ldw (n rounded up to a wavefront): a copy of the
        // model, then the state the loop carries -- x, targets, controls, v -- and the per-step u0 and
        // iteration counts.  Copies are row-wise with n elements per component, so a caller's ld > n
        // (a shard of a larger batch) is neither over-read nor over-written.
        //   0 A[4] 1 B[2I] 2 C[2] 3 Q[2] 4 R[I] 5 lo[I] 6 hi[I] 7 x[2] 8 targets[2H] 9 controls[HI] 10 v[HI] 11 u0[I]
        const int64_t ldw = (n + 63) / 64 * 64;
        const int comps[12] = {4, 2 * I, 2, 2, I, I, I, 2, 2 * H, H * I, H * I, I};
        const void* src[12] = {io->A, io->B, io->C, io->Q, io->R, io->lower, io->upper, io->x0, io->targets,
                               io->controls_inout, io->v_inout, nullptr};
        int64_t off[12], total = 0;
        for (int c = 0; c < 12; ++c) { off[c] = total; total += pad256((int64_t)comps[c] * ldw * es); }
        const int64_t o_iters = total; total += pad256(ldw * 4);
        // ... and the plant's arrays, behind everything the parent loop has
        const bool plant_abc = plant && plant->A;
        const int64_t o_pa = total; if (plant_abc) total += pad256(4 * ldw * es);
        const int64_t o_pb = total; if (plant_abc) total += pad256(2 * I * ldw * es);
        const int64_t o_pc = total; if (plant_abc) total += pad256(2 * ldw * es);
        rc = ensure(h, &h->roll, &h->roll_bytes, total);
        if (rc) return rc;
        if (polished) {
            rc = ensure(h, &h->grad_ws, &h->grad_ws_bytes, pad256(polish_scratch_bytes(I, H, n)));
            if (rc) return rc;
        }
        char* w = (char*)h->roll;
        for (int c = 0; c < 11; ++c) {
            if (src[c]) HIP_TRY(h, copy_rows(w + off[c], ldw * es, src[c], ld * es, n * es, comps[c], in_kind, s));
            else HIP_TRY(h, hipMemsetAsync(w + off[c], 0, (size_t)((int64_t)comps[c] * ldw * es), s));
        }
        // the per-step arrays: the kernels take the caller's DEVICE arrays, or the slots of HOST arrays
        StepArrays g = step_arrays(io, H, steps, (int)es, new_last_targets, plant, controls_out, states_out, iters_out,
                                   sequences_out, polished ? q : nullptr);
        if (host) {
            rc = stage_steps(h, &g, n, s);
            if (rc) return rc;
        }

        GeneralArgs a;
        std::memset(&a, 0, sizeof(a));
        a.n = n; a.ld = ldw; a.shift_controls = 1;
        a.A = w + off[0]; a.B = w + off[1]; a.C = w + off[2]; a.Q = w + off[3]; a.R = w + off[4];
        a.lo = w + off[5]; a.hi = w + off[6];
        a.x0 = w + off[7]; a.targets = w + off[8]; a.controls = w + off[9]; a.v = w + off[10]; a.u0 = w + off[11];
        a.iters = (int32_t*)(w + o_iters);
        a.flags = h->ws_words + 1;

        RolloutStepArgs r;
        std::memset(&r, 0, sizeof(r));
        r.n = n; r.ld = ldw; r.ld_out = g.ld_out; r.ld_nlt = g.ld_nlt; r.I = I; r.H = H; r.steps = steps;
        r.A = a.A; r.B = a.B; r.C = a.C;
        r.x = w + off[7]; r.targets = w + off[8]; r.controls = w + off[9]; r.new_last_targets = g.at(kStepNlt);
        r.controls_out = g.at(kStepCtrl); r.states_out = g.at(kStepStates);
        r.iters_step = a.iters; r.iters_out = g.at<int32_t>(kStepIters); r.sequences_out = g.at(kStepSeq);
        r.disturbance = g.at(kStepDist); r.ld_d = g.ld_d;
        if (plant_abc) {
            HIP_TRY(h, copy_rows(w + o_pa, ldw * es, plant->A, ld * es, n * es, 4, in_kind, s));
            HIP_TRY(h, copy_rows(w + o_pb, ldw * es, plant->B, ld * es, n * es, 2 * I, in_kind, s));
            HIP_TRY(h, copy_rows(w + o_pc, ldw * es, plant->C, ld * es, n * es, 2, in_kind, s));
            r.A = w + o_pa; r.B = w + o_pb; r.C = w + o_pc;
        }

        polish::Args pa;
        std::memset(&pa, 0, sizeof(pa));
        if (polished) {
            pa.n = n; pa.ld = ldw; pa.tol = q->tol; pa.max_rounds = q->max_rounds;
            pa.A = (const double*)a.A; pa.B = (const double*)a.B; pa.C = (const double*)a.C; pa.Q = (const double*)a.Q;
            pa.R = (const double*)a.R; pa.lo = (const double*)a.lo; pa.hi = (const double*)a.hi;
            pa.x0 = (const double*)r.x; pa.targets = (const double*)r.targets; pa.u = (double*)(w + off[9]);
        }

        Workspace ws;
        rc = prepare_workspace(h, algo, H, p->dtype, n, &ws, 1);
        if (rc) return rc;
        HIP_TRY(h, hipMemsetAsync(h->ws_words + 1, 0, sizeof(uint32_t), s));
        const Knobs kn = knobs_of(p);
        for (int st = 0; st < steps; ++st) {
            hipError_t e = dispatch_general(algo, I, H, p->dtype, a, kn, ws, s);
            if (e != hipSuccess) return hip_fail(h, e, "kernel launch");
            r.step = st;
            if (polished) {   // the step's rows of the polish outputs; the sequence is polished where the loop keeps it
                const int64_t at = (int64_t)st * g.ld_out;
                pa.status = g.at(kStepStatus) ? g.at<int32_t>(kStepStatus) + at : nullptr;
                pa.res_in = g.at(kStepRin) ? g.at<double>(kStepRin) + at : nullptr;
                pa.res_out = g.at(kStepRout) ? g.at<double>(kStepRout) + at : nullptr;
                e = launch_rollout_polish_step(I, pa, r, h->grad_ws, h->ws_words + 1, s);
            } else {
                e = launch_rollout_step(p->dtype, r, s);
            }
            if (e != hipSuccess) return hip_fail(h, e, "rollout step launch");
        }
        // controller state back to the caller
        if (io->controls_inout)
            HIP_TRY(h, copy_rows(io->controls_inout, ld * es, w + off[9], ldw * es, n * es, H * I, out_kind, s));
        if (io->v_inout) HIP_TRY(h, copy_rows(io->v_inout, ld * es, w + off[10], ldw * es, n * es, H * I, out_kind, s));
        if (host) {
            rc = stage_out(h, g.t, kStepCount, n, s);
            if (rc) return rc;
        }
        rc = order.end();
        if (rc) return rc;
        return finish_flags(h, flags_out, s);
    });
}

}  // namespace

int tpc_mpc_rollout_polished(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                             int32_t steps, const void* new_last_targets, const tpc_mpc_polish* q,
                             void* controls_out, void* states_out, int32_t* iters_out, void* sequences_out,
                             uint32_t* flags_out, int mem, void* stream) {
    return rollout_impl(h, p, io, steps, new_last_targets, controls_out, states_out, iters_out, sequences_out, false,
                        true, q, flags_out, mem, stream);
}

int tpc_mpc_rollout(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                    int32_t steps, const void* new_last_targets, void* controls_out,
                    void* states_out, int32_t* iters_out, uint32_t* flags_out, int mem,
                    void* stream) {
    return rollout_impl(h, p, io, steps, new_last_targets, controls_out, states_out, iters_out, nullptr, false,
                        false, nullptr, flags_out, mem, stream);
}

int tpc_mpc_rollout_record(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                           int32_t steps, const void* new_last_targets, void* controls_out,
                           void* states_out, int32_t* iters_out, void* sequences_out, uint32_t* flags_out,
                           int mem, void* stream) {
    return rollout_impl(h, p, io, steps, new_last_targets, controls_out, states_out, iters_out, sequences_out, true,
                        false, nullptr, flags_out, mem, stream);
}

// The Newton-first closed loop (include/tpc_mpc.h) on newton_two_phase: phase 1 is ONE launch for the whole loop
// (mpc_rollout_newton.hip); the fallback is rollout_impl's polished mode from step 0 on the gathered rows of the
// working set.  A host-only handle runs phase 1 on the calling thread.
// (plant: tpc_mpc_rollout_plant, which has checked it; null: tpc_mpc_rollout_newton)
static int rollout_newton_impl(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, int32_t steps,
                               const void* new_last_targets, const tpc_mpc_polish* q, int32_t fallback,
                               void* controls_out, void* states_out, int32_t* iters_out, void* sequences_out,
                               int32_t* first_unverified, uint32_t* flags_out, int mem, void* stream,
                               const tpc_mpc_plant* plant) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_rollout_newton");
        rc = check_general_io(h, io, mem);
        if (!rc) rc = check_polish(h, q);
        if (!rc) rc = check_fallback(h, fallback);
        if (!rc) rc = check_steps(h, steps);
        if (rc) return rc;
        const bool solve = fallback == TPC_MPC_NEWTON_FALLBACK_SOLVE;
        rc = check_host_only_newton(h, solve, mem);
        if (rc) return rc;
        if (io->n == 0 || steps == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        rc = check_model(h, io, controls_out != nullptr);
        if (rc) return rc;
        const int I = io->inputs, H = p->horizon;
        const int64_t n = io->n, ld = io->ld;
        // the working set: a copy of the model, then x0, targets, controls and v AS GIVEN (what the fallback restarts
        // from), row after row with one leading dimension
        //   0 A[4] 1 B[2I] 2 C[2] 3 Q[2] 4 R[I] 5 lo[I] 6 hi[I] 7 x[2] 8 targets[2H] 9 controls[HI] 10 v[HI]
        //   11 Ap[4] 12 Bp[2I] 13 Cp[2]: the plant's arrays when tpc_mpc_rollout_plant gave some (no rows otherwise)
        const bool plant_abc = plant && plant->A, plant_d = plant && plant->disturbance;
        const int comps[14] = {4, 2 * I, 2, 2, I, I, I, 2, 2 * H, H * I, H * I,
                               plant_abc ? 4 : 0, plant_abc ? 2 * I : 0, plant_abc ? 2 : 0};
        const void* src[14] = {io->A, io->B, io->C, io->Q, io->R, io->lower, io->upper, io->x0, io->targets,
                               io->controls_inout, io->v_inout, plant_abc ? plant->A : nullptr,
                               plant_abc ? plant->B : nullptr, plant_abc ? plant->C : nullptr};
        int64_t row[15];
        row[0] = 0;
        for (int c = 0; c < 14; ++c) row[c + 1] = row[c] + comps[c];
        const int64_t rows_in = row[14], rows_work = 2 + 2 * H + H * I;   // ... and the state the loop carries: x, targets, controls

        NewtonArgs a;
        std::memset(&a, 0, sizeof(a));
        a.p.n = n; a.p.tol = q->tol; a.p.max_rounds = q->max_rounds;
        a.r.n = n; a.r.I = I; a.r.H = H; a.r.steps = steps;
        a.raise_not_polished = solve ? 0 : 1;
        a.plant = (plant_abc || plant_d) ? 1 : 0;
        auto bind = [&](char* w, int64_t ldw) {   // w: rows_in rows as given, then rows_work rows of carried state
            auto at = [&](int64_t r) { return (double*)(w + r * ldw * 8); };
            a.p.ld = a.r.ld = ldw;
            a.p.A = at(row[0]); a.p.B = at(row[1]); a.p.C = at(row[2]); a.p.Q = at(row[3]); a.p.R = at(row[4]);
            a.p.lo = at(row[5]); a.p.hi = at(row[6]);
            a.p.x0 = at(rows_in); a.p.targets = at(rows_in + 2); a.p.u = at(rows_in + 2 + 2 * H);
            a.r.A = a.p.A; a.r.B = a.p.B; a.r.C = a.p.C;
            if (plant_abc) { a.r.A = at(row[11]); a.r.B = at(row[12]); a.r.C = at(row[13]); }
            a.r.x = at(rows_in); a.r.targets = at(rows_in + 2); a.r.controls = a.p.u;
        };

        if (h->host_only) {   // on the calling thread, outputs straight into the caller's arrays
            std::vector<double> w((size_t)((rows_in + rows_work) * n), 0.0);
            std::vector<int32_t> fu(first_unverified ? 0 : (size_t)n);
            for (int c = 0; c < 10; ++c)
                if (src[c])
                    for (int64_t r = 0; r < comps[c]; ++r)
                        std::memcpy(&w[(size_t)((row[c] + r) * n)], (const double*)src[c] + r * ld, (size_t)n * 8);
            for (int c = 11; c < 14; ++c)
                for (int64_t r = 0; r < comps[c]; ++r)
                    std::memcpy(&w[(size_t)((row[c] + r) * n)], (const double*)src[c] + r * ld, (size_t)n * 8);
            if (plant_d) { a.r.disturbance = plant->disturbance; a.r.ld_d = plant->ld_d; }
            std::memcpy(&w[(size_t)(rows_in * n)], &w[(size_t)(row[7] * n)], (size_t)(rows_work * n) * 8);
            bind((char*)w.data(), n);
            a.r.ld_out = a.r.ld_nlt = ld;
            a.r.new_last_targets = new_last_targets;
            a.r.controls_out = controls_out; a.r.states_out = states_out; a.r.iters_out = iters_out;
            a.r.sequences_out = sequences_out;
            a.p.status = q->status; a.p.res_in = (double*)q->residual_in; a.p.res_out = (double*)q->residual_out;
            a.first_unverified = first_unverified ? first_unverified : fu.data();
            const uint32_t f = rollout_newton_host(I, a);
            for (int64_t r = 0; r < H * I; ++r) {
                if (io->controls_inout) std::memcpy((double*)io->controls_inout + r * ld, a.p.u + r * n, (size_t)n * 8);
                if (io->v_inout) std::memcpy((double*)io->v_inout + r * ld, a.p.u + r * n, (size_t)n * 8);
            }
            if (flags_out) *flags_out = f;
            return TPC_MPC_OK;
        }

        const bool host = mem == TPC_MPC_HOST;
        const hipMemcpyKind in_kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        const hipMemcpyKind out_kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        const int64_t ldw = stage_ld(n), S = steps;
        const int64_t o_fu = (rows_in + rows_work) * ldw * 8;   // first_unverified's row; the frame's queue follows it
        // the per-step arrays: the kernels take the caller's DEVICE arrays, or the slots of HOST arrays
        StepArrays g = step_arrays(io, H, steps, 8, new_last_targets, plant, controls_out, states_out, iters_out,
                                   sequences_out, q);
        StepOutputs out{};                               // ... as phase 1 binds them
        char *d_cfinal = nullptr, *d_vfinal = nullptr;   // the last step's sequence: controls out, and v out
        return newton_two_phase(
            h, n, solve, mem, stream, flags_out, o_fu + ldw * 4, polish_scratch_bytes(I, H, n), g.t, kStepCount,
            [&](const NewtonPhase& f) -> int {   // the working set
                char* w = f.ws;
                for (int c = 0; c < 14; ++c) {
                    if (comps[c] == 0) continue;
                    if (src[c]) HIP_TRY(h, copy_rows(w + row[c] * ldw * 8, ldw * 8, src[c], ld * 8, n * 8, comps[c], in_kind, f.s));
                    else HIP_TRY(h, hipMemsetAsync(w + row[c] * ldw * 8, 0, (size_t)(comps[c] * ldw * 8), f.s));
                }
                HIP_TRY(h, hipMemcpyAsync(w + rows_in * ldw * 8, w + row[7] * ldw * 8, (size_t)(rows_work * ldw * 8),
                                          hipMemcpyDeviceToDevice, f.s));
                return TPC_MPC_OK;
            },
            [&](const NewtonPhase& f) {   // phase 1
                if (f.staged) staged_step_lds(&g, n);
                out = StepOutputs{g.at(kStepCtrl), g.at(kStepStates), g.at(kStepSeq), g.at(kStepRin), g.at(kStepRout),
                                  g.at<int32_t>(kStepIters), g.at<int32_t>(kStepStatus)};
                bind(f.ws, ldw);
                a.r.ld_out = g.ld_out; a.r.ld_nlt = g.ld_nlt;
                a.r.new_last_targets = g.at(kStepNlt);
                a.r.disturbance = g.at(kStepDist); a.r.ld_d = g.ld_d;
                a.r.controls_out = out.ctrl; a.r.states_out = out.states; a.r.iters_out = out.iters;
                a.r.sequences_out = out.seq;
                a.p.status = out.status; a.p.res_in = (double*)out.rin; a.p.res_out = (double*)out.rout;
                a.first_unverified = (int32_t*)(f.ws + o_fu);
                a.fb_index = f.fb_index; a.fb_count = f.fb_count;
                d_cfinal = d_vfinal = f.ws + (rows_in + 2 + 2 * H) * ldw * 8;
                return rollout_newton(I, a, h->grad_ws, f.flags, f.s);
            },
            [&](const NewtonPhase& f, int64_t cnt, int64_t ldc) -> int {   // the fallback: the polished loop from step 0
                // the compact batch: the rows_in rows of the working set, new_last_targets, every output of the
                // polished loop, the disturbance
                const void *d_nlt = g.at(kStepNlt), *d_dist = g.at(kStepDist);
                FallbackRows L(ldc);
                L.take(true, rows_in);
                const int64_t r_nlt = L.take(d_nlt != nullptr, S * 2);
                const StepRows r_out = take_step_rows(&L, out, I, H, S);
                const int64_t r_dist = L.take(d_dist != nullptr, S * 2);
                int rc = L.reserve(h, 2 * S);
                if (rc) return rc;
                const StepOutputs fo = step_outputs_at(L, r_out, out, S, true);

                NewtonMove gm{cnt, f.fb_index, 0, {}};
                gm.set[gm.sets++] = NewtonRows{f.ws, L.fb, rows_in, ldw, ldc, 8};
                if (d_nlt) gm.set[gm.sets++] = NewtonRows{d_nlt, L.at(r_nlt), S * 2, g.ld_nlt, ldc, 8};
                if (d_dist) gm.set[gm.sets++] = NewtonRows{d_dist, L.at(r_dist), S * 2, g.ld_d, ldc, 8};
                hipError_t e = rollout_newton_move(gm, false, f.s);
                if (e != hipSuccess) return hip_fail(h, e, "gather launch");

                tpc_mpc_general_io io2 = fallback_io(L, I, cnt, row);
                io2.controls_inout = L.at(row[9]); io2.v_inout = L.at(row[10]);
                tpc_mpc_polish q2 = *q;
                q2.status = fo.status; q2.residual_in = fo.rin; q2.residual_out = fo.rout;
                // ... against the same plant: its gathered arrays and disturbance rows
                tpc_mpc_plant plant2{};
                if (plant_abc) { plant2.A = L.at(row[11]); plant2.B = L.at(row[12]); plant2.C = L.at(row[13]); }
                plant2.disturbance = L.at(r_dist); plant2.ld_d = ldc;
                rc = rollout_impl(h, p, &io2, steps, L.at(r_nlt), fo.ctrl, fo.states, fo.iters, fo.seq, false, true, &q2,
                                  nullptr, TPC_MPC_DEVICE, stream, a.plant ? &plant2 : nullptr);
                if (rc) return rc;

                if (io->v_inout) {   // v out: the sequence for a Newton-only instance, the polished loop's v for the others
                    d_vfinal = f.ws + row[10] * ldw * 8;
                    HIP_TRY(h, hipMemcpyAsync(d_vfinal, d_cfinal, (size_t)((int64_t)H * I * ldw * 8), hipMemcpyDeviceToDevice, f.s));
                }
                NewtonMove sc = step_scatter(cnt, f.fb_index, fo, out, I, H, S, ldc, g.ld_out);
                sc.set[sc.sets++] = NewtonRows{L.at(row[9]), d_cfinal, (int64_t)H * I, ldc, ldw, 8};
                if (io->v_inout) sc.set[sc.sets++] = NewtonRows{L.at(row[10]), d_vfinal, (int64_t)H * I, ldc, ldw, 8};
                e = rollout_newton_move(sc, true, f.s);
                if (e != hipSuccess) return hip_fail(h, e, "scatter launch");
                return TPC_MPC_OK;
            },
            [&](const NewtonPhase& f) -> int {   // controller state and first_unverified back to the caller
                if (io->controls_inout) HIP_TRY(h, copy_rows(io->controls_inout, ld * 8, d_cfinal, ldw * 8, n * 8, H * I, out_kind, f.s));
                if (io->v_inout) HIP_TRY(h, copy_rows(io->v_inout, ld * 8, d_vfinal, ldw * 8, n * 8, H * I, out_kind, f.s));
                if (first_unverified) HIP_TRY(h, hipMemcpyAsync(first_unverified, f.ws + o_fu, (size_t)n * 4, out_kind, f.s));
                return TPC_MPC_OK;
            });
    });
}

int tpc_mpc_rollout_newton(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, int32_t steps,
                           const void* new_last_targets, const tpc_mpc_polish* q, int32_t fallback, void* controls_out,
                           void* states_out, int32_t* iters_out, void* sequences_out, int32_t* first_unverified,
                           uint32_t* flags_out, int mem, void* stream) {
    return rollout_newton_impl(h, p, io, steps, new_last_targets, q, fallback, controls_out, states_out, iters_out,
                               sequences_out, first_unverified, flags_out, mem, stream, nullptr);
}

// The exact compact solve (include/tpc_mpc.h) on newton_two_phase: phase 1 is ONE launch, three rows in and two (+2H)
// out (mpc_newton_compact.hip); the fallback expands the queued instances to the general form on the device and runs
// tpc_mpc_solve_batch_general and tpc_mpc_polish_batch_general on them.  A host-only handle runs phase 1 on the calling
// thread.
// `rows`: tpc_mpc_solve_batch_compact_exact_rows -- the ten model values per instance from params_rows ([10], ld n, in
// `mem` like v), p's own neither read nor checked.
// `warm`: tpc_mpc_solve_batch_compact_exact_from -- phase 1 starts from `start` ([H*2], ld n, in `mem`) on the warm
// kernels; everything after phase 1 is the same code.
static int compact_exact_impl(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v, const void* delta_y,
                              const void* delta_phi, bool rows, const void* params_rows, bool warm, const void* start,
                              const tpc_mpc_polish* q,
                              int32_t fallback, void* steering_front, void* steering_rear, void* sequence_out,
                              int32_t* fell_back, uint32_t* flags_out, int mem, void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64)
            return fp64_only(h, warm   ? "tpc_mpc_solve_batch_compact_exact_from"
                                : rows ? "tpc_mpc_solve_batch_compact_exact_rows"
                                       : "tpc_mpc_solve_batch_compact_exact");
        if (!rows) {
            rc = check_compact_model(h, p);
            if (rc) return rc;
        }
        rc = check_batch(h, n, mem);
        if (!rc) rc = check_polish(h, q);
        if (!rc) rc = check_fallback(h, fallback);
        if (rc) return rc;
        const bool solve = fallback == TPC_MPC_NEWTON_FALLBACK_SOLVE;
        rc = check_host_only_newton(h, solve, mem);
        if (rc) return rc;
        if (n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        if (!v || !delta_y || !delta_phi || !steering_front || !steering_rear)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
        if (rows && !params_rows) return fail(h, TPC_MPC_ERR_BAD_ARG, "null params_rows");
        if (warm && !start) return fail(h, TPC_MPC_ERR_BAD_ARG, "null start");
        const int H = p->horizon;

        cexact::Args a;
        std::memset(&a, 0, sizeof(a));
        a.n = n;
        if (!rows) bind_compact_model(&a, p);
        a.tol = q->tol; a.max_rounds = q->max_rounds;
        a.raise_not_polished = solve ? 0 : 1;
        // the call's arrays, every one with the leading dimension n in the caller's memory
        enum { kV, kDy, kDphi, kParams, kStart, kFront, kRear, kSeq, kRin, kRout, kStatus, kFell, kCount };
        StagedArray t[kCount] = {staged(v, kStageIn, 1, n), staged(delta_y, kStageIn, 1, n), staged(delta_phi, kStageIn, 1, n),
                                 staged(rows ? params_rows : nullptr, kStageIn, cgrad::kParams, n),
                                 staged(warm ? start : nullptr, kStageIn, 2 * H, n),
                                 staged(steering_front, kStageOut, 1, n), staged(steering_rear, kStageOut, 1, n),
                                 staged(sequence_out, kStageOut, 2 * H, n), staged(q->residual_in, kStageOut, 1, n),
                                 staged(q->residual_out, kStageOut, 1, n), staged(q->status, kStageOut, 1, n, 4),
                                 staged(fell_back, kStageOut, 1, n, 4)};
        // what the kernels take: the caller's arrays (DEVICE, or a host-only handle) or the slots of HOST arrays
        auto bind = [&](int64_t ld) {
            a.v = (const double*)t[kV].dev; a.dy = (const double*)t[kDy].dev; a.dphi = (const double*)t[kDphi].dev;
            a.params = (const double*)t[kParams].dev; a.start = (const double*)t[kStart].dev;
            a.front = (double*)t[kFront].dev; a.rear = (double*)t[kRear].dev; a.seq = (double*)t[kSeq].dev;
            a.res_in = (double*)t[kRin].dev; a.res_out = (double*)t[kRout].dev;
            a.status = (int32_t*)t[kStatus].dev; a.fell_back = (int32_t*)t[kFell].dev;
            a.ld_params = a.ld_start = a.ld_seq = ld;
        };

        if (h->host_only) {   // on the calling thread, straight from and into the caller's arrays
            bind(n);
            const uint32_t f = compact_exact_host(H, a);
            if (flags_out) *flags_out = f;
            return TPC_MPC_OK;
        }

        return newton_two_phase(
            h, n, solve, mem, stream, flags_out, 0, compact_exact_in_registers(H) ? 0 : polish_scratch_bytes(2, H, n), t,
            kCount, newton_nothing,
            [&](const NewtonPhase& f) {   // phase 1
                bind(f.staged ? stage_ld(n) : n);
                a.fb_index = f.fb_index; a.fb_count = f.fb_count;
                return compact_exact(H, a, h->grad_ws, f.flags, f.s);
            },
            [&](const NewtonPhase& f, int64_t cnt, int64_t ldc) -> int {   // the fallback: the solve, then the polish
                // the compact batch: the general form of the queued instances, then what the solve and the polish
                // return for them
                FallbackRows L(ldc);
                const int64_t r_model = L.take(true, compact_model_rows(H)), r_ctrl = L.take(true, 2 * H);
                const int64_t r_u0 = L.take(true, 2), r_rin = L.take(true, 1), r_rout = L.take(true, 1);
                int rc = L.reserve(h, 1);
                if (rc) return rc;
                CompactExactBatch b{};
                tpc_mpc_general_io io2 = fallback_compact_model(L, r_model, H, cnt, f.fb_index, &b);
                b.controls = L.at(r_ctrl); b.u0 = L.at(r_u0); b.res_in = L.at(r_rin); b.res_out = L.at(r_rout);
                b.status = L.at32(true, 0);
                hipError_t e = compact_exact_gather(a, b, f.s);
                if (e != hipSuccess) return hip_fail(h, e, "gather launch");

                io2.controls_inout = b.controls; io2.u0 = b.u0;
                tpc_mpc_polish q2 = *q;
                q2.status = b.status; q2.residual_in = b.res_in; q2.residual_out = b.res_out;
                // the polish resets the handle's flag word like the solve: the solve's flags join phase 1's first
                rc = tpc_mpc_solve_batch_general(h, p, &io2, nullptr, TPC_MPC_DEVICE, stream);
                if (rc) return rc;
                e = rollout_newton_merge_flags(f.flags, h->ws_words + 1, f.s);
                if (e != hipSuccess) return hip_fail(h, e, "flag merge launch");
                rc = tpc_mpc_polish_batch_general(h, p, &io2, &q2, nullptr, TPC_MPC_DEVICE, stream);
                if (rc) return rc;
                e = compact_exact_scatter(a, b, f.s);
                if (e != hipSuccess) return hip_fail(h, e, "scatter launch");
                return TPC_MPC_OK;
            },
            newton_nothing);
    });
}

int tpc_mpc_solve_batch_compact_exact(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                      const void* delta_y, const void* delta_phi, const tpc_mpc_polish* q,
                                      int32_t fallback, void* steering_front, void* steering_rear, void* sequence_out,
                                      int32_t* fell_back, uint32_t* flags_out, int mem, void* stream) {
    return compact_exact_impl(h, p, n, v, delta_y, delta_phi, false, nullptr, false, nullptr, q, fallback,
                              steering_front, steering_rear, sequence_out, fell_back, flags_out, mem, stream);
}

int tpc_mpc_solve_batch_compact_exact_rows(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                           const void* delta_y, const void* delta_phi, const void* params_rows,
                                           const tpc_mpc_polish* q, int32_t fallback, void* steering_front,
                                           void* steering_rear, void* sequence_out, int32_t* fell_back,
                                           uint32_t* flags_out, int mem, void* stream) {
    return compact_exact_impl(h, p, n, v, delta_y, delta_phi, true, params_rows, false, nullptr, q, fallback,
                              steering_front, steering_rear, sequence_out, fell_back, flags_out, mem, stream);
}

int tpc_mpc_solve_batch_compact_exact_from(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                           const void* delta_y, const void* delta_phi, const void* params_rows,
                                           const void* start, const tpc_mpc_polish* q, int32_t fallback,
                                           void* steering_front, void* steering_rear, void* sequence_out,
                                           int32_t* fell_back, uint32_t* flags_out, int mem, void* stream) {
    return compact_exact_impl(h, p, n, v, delta_y, delta_phi, params_rows != nullptr, params_rows, true, start, q,
                              fallback, steering_front, steering_rear, sequence_out, fell_back, flags_out, mem, stream);
}

// The compact closed loop (include/tpc_mpc.h) on newton_two_phase: phase 1 is ONE launch for the whole loop, three
// (+ 2) rows in and the per-step rows out (mpc_compact_loop.hip); the fallback expands the queued instances to the
// general form on the device and runs rollout_impl's polished mode from step 0 on them, whose rows
// rollout_newton_move scatters back.  A host-only handle runs phase 1 on the calling thread.
int tpc_mpc_rollout_compact_exact(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                  const void* delta_y, const void* delta_phi, const void* x0, int32_t steps,
                                  const tpc_mpc_polish* q, int32_t fallback, void* controls_out, void* states_out,
                                  void* sequences_out, int32_t* first_unverified, uint32_t* flags_out, int mem,
                                  void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_rollout_compact_exact");
        rc = check_compact_model(h, p);
        if (rc) return rc;
        rc = check_batch(h, n, mem);
        if (!rc) rc = check_polish(h, q);
        if (!rc) rc = check_fallback(h, fallback);
        if (!rc) rc = check_steps(h, steps);
        if (rc) return rc;
        const bool solve = fallback == TPC_MPC_NEWTON_FALLBACK_SOLVE;
        rc = check_host_only_newton(h, solve, mem);
        if (rc) return rc;
        if (n == 0 || steps == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        if (!v || !delta_y || !delta_phi || !controls_out) return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
        const int H = p->horizon;
        const int64_t S = steps;

        cloop::Args a;
        std::memset(&a, 0, sizeof(a));
        a.c.n = n;
        bind_compact_model(&a.c, p);
        a.c.tol = q->tol; a.c.max_rounds = q->max_rounds;
        a.c.raise_not_polished = solve ? 0 : 1;
        a.steps = steps;
        // the call's arrays, every one with the leading dimension n in the caller's memory
        enum { kV, kDy, kDphi, kX0, kCtrl, kStates, kSeq, kRin, kRout, kStatus, kFirst, kCount };
        StagedArray t[kCount] = {staged(v, kStageIn, 1, n), staged(delta_y, kStageIn, 1, n), staged(delta_phi, kStageIn, 1, n),
                                 staged(x0, kStageIn, 2, n), staged(controls_out, kStageOut, S * 2, n),
                                 staged(states_out, kStageOut, S * 2, n), staged(sequences_out, kStageOut, S * H * 2, n),
                                 staged(q->residual_in, kStageOut, S, n), staged(q->residual_out, kStageOut, S, n),
                                 staged(q->status, kStageOut, S, n, 4), staged(first_unverified, kStageOut, 1, n, 4)};
        // what the kernels take: the caller's arrays (DEVICE, or a host-only handle) or the slots of HOST arrays
        auto bind = [&](int64_t ld) {
            a.c.v = (const double*)t[kV].dev; a.c.dy = (const double*)t[kDy].dev; a.c.dphi = (const double*)t[kDphi].dev;
            a.x0 = (const double*)t[kX0].dev;
            a.controls = (double*)t[kCtrl].dev; a.states = (double*)t[kStates].dev; a.sequences = (double*)t[kSeq].dev;
            a.res_in = (double*)t[kRin].dev; a.res_out = (double*)t[kRout].dev;
            a.status = (int32_t*)t[kStatus].dev; a.first = (int32_t*)t[kFirst].dev;
            a.ld_x0 = a.ld_out = ld;
        };

        if (h->host_only) {   // on the calling thread, straight from and into the caller's arrays
            bind(n);
            const uint32_t f = compact_loop_host(H, a);
            if (flags_out) *flags_out = f;
            return TPC_MPC_OK;
        }

        int64_t ld = n;       // ... of the arrays the kernels take, and those as the polished loop's outputs
        StepOutputs out{};
        return newton_two_phase(
            h, n, solve, mem, stream, flags_out, 0, compact_loop_in_registers(H) ? 0 : polish_scratch_bytes(2, H, n), t,
            kCount, newton_nothing,
            [&](const NewtonPhase& f) {   // phase 1
                if (f.staged) ld = stage_ld(n);
                bind(ld);
                out = StepOutputs{a.controls, a.states, a.sequences, a.res_in, a.res_out, nullptr, a.status};
                a.c.fb_index = f.fb_index; a.c.fb_count = f.fb_count;
                return compact_loop(H, a, h->grad_ws, f.flags, f.s);
            },
            [&](const NewtonPhase& f, int64_t cnt, int64_t ldc) -> int {   // the fallback: the polished loop from step 0
                // the compact batch: the general form of the queued instances, then every output of the polished
                // loop that the caller asked for
                FallbackRows L(ldc);
                const int64_t r_model = L.take(true, compact_model_rows(H));
                const StepRows r_out = take_step_rows(&L, out, 2, H, S);
                int rc = L.reserve(h, S);
                if (rc) return rc;
                const StepOutputs fo = step_outputs_at(L, r_out, out, S, false);
                CompactLoopBatch b{};
                const tpc_mpc_general_io io2 = fallback_compact_model(L, r_model, H, cnt, f.fb_index, &b);
                hipError_t e = compact_loop_gather(a, b, f.s);
                if (e != hipSuccess) return hip_fail(h, e, "gather launch");

                tpc_mpc_polish q2 = *q;
                q2.status = fo.status; q2.residual_in = fo.rin; q2.residual_out = fo.rout;
                rc = rollout_impl(h, p, &io2, steps, nullptr, fo.ctrl, fo.states, nullptr, fo.seq, false, true, &q2,
                                  nullptr, TPC_MPC_DEVICE, stream);
                if (rc) return rc;
                e = rollout_newton_move(step_scatter(cnt, f.fb_index, fo, out, 2, H, S, ldc, ld), true, f.s);
                if (e != hipSuccess) return hip_fail(h, e, "scatter launch");
                return TPC_MPC_OK;
            },
            newton_nothing);
    });
}

// The backward pass of the exact compact solve: one launch of the adjoint sweep on the model built from v
// (mpc_compact_grad.hip), and with dparams one more, single-block launch that sums the blocks' partial rows.  The
// per-step workspace (none at the register kernels' horizons) and the partial rows live in the gradient workspace; a
// one-launch entry like the general backward pass (staged_run).
// `rows`: tpc_mpc_solve_batch_compact_exact_rows_backward, as compact_exact_impl takes params_rows.
static int compact_exact_backward_impl(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                       const void* delta_y, const void* delta_phi, bool rows, const void* params_rows,
                                       const void* sequence, const int32_t* status, const tpc_mpc_compact_grad* g,
                                       uint32_t* flags_out, int mem, void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64)
            return fp64_only(h, rows ? "tpc_mpc_solve_batch_compact_exact_rows_backward"
                                     : "tpc_mpc_solve_batch_compact_exact_backward");
        if (!rows) {
            rc = check_compact_model(h, p);
            if (rc) return rc;
        }
        rc = check_batch(h, n, mem);
        if (rc) return rc;
        if (!g) return fail(h, TPC_MPC_ERR_BAD_ARG, "null gradient struct");
        rc = check_host_only_pass(h, mem, "backward pass");
        if (rc) return rc;
        constexpr int kP = cgrad::kParams;
        if (n == 0) return zero_dparams(h, g->dparams, kP, flags_out, mem, stream);
        if (!v || !delta_y || !delta_phi) return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
        if (!sequence) return fail(h, TPC_MPC_ERR_BAD_ARG, "null sequence");
        if (rows && !params_rows) return fail(h, TPC_MPC_ERR_BAD_ARG, "null params_rows");
        const int H = p->horizon;
        // the arrays in order: 9 inputs (params_rows and status, int32, may be null like the upstream gradients), then
        // 6 outputs; dparams is one row of kP sums, not one element per instance
        const void* src[9] = {rows ? params_rows : nullptr, v, delta_y, delta_phi, sequence, g->grad_front, g->grad_rear,
                              g->grad_sequence, status};
        void* dst[6] = {g->dv, g->ddelta_y, g->ddelta_phi, g->dparams_rows, g->kkt_residual, g->dparams};
        const int64_t comps[15] = {kP, 1, 1, 1, 2 * H, 1, 1, 2 * H, 1, 1, 1, 1, kP, 1, 1};
        int width[15] = {0};
        width[8] = 4;
        int64_t elems[15] = {0};
        elems[14] = kP;
        StagedExtra x;
        x.width = width;
        x.elems = elems;
        // the gradient workspace: the per-step slots, then the blocks' partial rows
        const int64_t ws_b = pad256(compact_grad_scratch_bytes(H, n));
        const int64_t part_b = g->dparams ? pad256(kP * compact_grad_blocks(n) * 8) : 0;
        return staged_run(h, n, n, mem, stream, flags_out, ws_b + part_b, src, dst, comps,
                          [&](int64_t ld, const void* const* in, void* const* out, hipStream_t s, uint32_t* hf) {
                              cgrad::Args a;
                              std::memset(&a, 0, sizeof(a));
                              a.n = n; a.ld = ld;
                              if (!rows) bind_compact_model(&a, p);
                              a.params = (const double*)in[0];
                              a.v = (const double*)in[1]; a.dy = (const double*)in[2]; a.dphi = (const double*)in[3];
                              a.seq = (const double*)in[4]; a.gf = (const double*)in[5]; a.gr = (const double*)in[6];
                              a.gs = (const double*)in[7]; a.status = (const int32_t*)in[8];
                              a.dv = (double*)out[0]; a.ddy = (double*)out[1]; a.ddphi = (double*)out[2];
                              a.rows = (double*)out[3]; a.kkt = (double*)out[4];
                              if (hf) { *hf = compact_grad_host(H, a, (double*)out[5]); return hipSuccess; }
                              double* partials = out[5] ? (double*)((char*)h->grad_ws + ws_b) : nullptr;
                              return compact_grad(H, a, h->grad_ws, partials, (double*)out[5], h->ws_words + 1, s);
                          },
                          x);
    });
}

int tpc_mpc_solve_batch_compact_exact_backward(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                               const void* delta_y, const void* delta_phi, const void* sequence,
                                               const int32_t* status, const tpc_mpc_compact_grad* g,
                                               uint32_t* flags_out, int mem, void* stream) {
    return compact_exact_backward_impl(h, p, n, v, delta_y, delta_phi, false, nullptr, sequence, status, g, flags_out,
                                       mem, stream);
}

int tpc_mpc_solve_batch_compact_exact_rows_backward(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n,
                                                    const void* v, const void* delta_y, const void* delta_phi,
                                                    const void* params_rows, const void* sequence,
                                                    const int32_t* status, const tpc_mpc_compact_grad* g,
                                                    uint32_t* flags_out, int mem, void* stream) {
    return compact_exact_backward_impl(h, p, n, v, delta_y, delta_phi, true, params_rows, sequence, status, g,
                                       flags_out, mem, stream);
}

// The backward pass of the compact closed loop: one launch of the reverse sweep over the steps on the model built from v
// (mpc_compact_loop_grad.hip), and with dparams the single-block launch that sums the blocks' partial rows
// (compact_grad_reduce).  One step's workspace (none at the register kernels' horizons) and the partial rows live in the
// gradient workspace; a one-launch entry like the single solve's backward pass (staged_run).
int tpc_mpc_rollout_compact_exact_backward(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                           const void* delta_y, const void* delta_phi, const void* x0, int32_t steps,
                                           const void* sequences, const void* states, const int32_t* status,
                                           const tpc_mpc_compact_loop_grad* g, uint32_t* flags_out, int mem,
                                           void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_rollout_compact_exact_backward");
        rc = check_compact_model(h, p);
        if (rc) return rc;
        rc = check_batch(h, n, mem);
        if (rc) return rc;
        if (!g) return fail(h, TPC_MPC_ERR_BAD_ARG, "null gradient struct");
        rc = check_steps(h, steps);
        if (rc) return rc;
        rc = check_host_only_pass(h, mem, "backward pass");
        if (rc) return rc;
        constexpr int kP = cloopgrad::kParams;
        if (n == 0 || steps == 0) return zero_dparams(h, g->dparams, kP, flags_out, mem, stream);
        if (!v || !delta_y || !delta_phi) return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
        if (!sequences || !states) return fail(h, TPC_MPC_ERR_BAD_ARG, "null sequences / states");
        const int H = p->horizon;
        const int64_t S = steps;
        // the arrays in order: 9 inputs (x0, status -- int32 -- and the upstream gradients may be null), then 7 outputs;
        // dparams is one row of kP sums, not one element per instance
        constexpr int kIn = 9, kOut = 7;
        const void* src[kIn] = {v, delta_y, delta_phi, x0, sequences, states, status, g->grad_controls, g->grad_states};
        void* dst[kOut] = {g->dv, g->ddelta_y, g->ddelta_phi, g->dx0, g->dparams_rows, g->kkt_residual, g->dparams};
        const int64_t comps[kIn + kOut] = {1, 1, 1, 2, S * H * 2, S * 2, S, S * 2, S * 2, 1, 1, 1, 2, kP, 1, 1};
        int width[kIn + kOut] = {0};
        width[6] = 4;
        int64_t elems[kIn + kOut] = {0};
        elems[kIn + 6] = kP;
        StagedExtra x;
        x.width = width;
        x.elems = elems;
        // the gradient workspace: one step's slots, then the blocks' partial rows
        const int64_t ws_b = pad256(cloop_grad_scratch_bytes(H, n));
        const int64_t part_b = g->dparams ? pad256(kP * cloop_grad_blocks(n) * 8) : 0;
        return staged_run(h, n, n, mem, stream, flags_out, ws_b + part_b, src, dst, comps,
                          [&](int64_t ld, const void* const* in, void* const* out, hipStream_t s, uint32_t* hf) {
                              cloopgrad::Args a;
                              std::memset(&a, 0, sizeof(a));
                              a.n = n; a.ld = ld; a.steps = steps;
                              bind_compact_model(&a, p);
                              a.v = (const double*)in[0]; a.dy = (const double*)in[1]; a.dphi = (const double*)in[2];
                              a.x0 = (const double*)in[3]; a.seq = (const double*)in[4];
                              a.states = (const double*)in[5]; a.status = (const int32_t*)in[6];
                              a.gu = (const double*)in[7]; a.gx = (const double*)in[8];
                              a.dv = (double*)out[0]; a.ddy = (double*)out[1]; a.ddphi = (double*)out[2];
                              a.dx0 = (double*)out[3]; a.rows = (double*)out[4]; a.kkt = (double*)out[5];
                              if (hf) { *hf = cloop_grad_host(H, a, (double*)out[6]); return hipSuccess; }
                              double* partials = out[6] ? (double*)((char*)h->grad_ws + ws_b) : nullptr;
                              return cloop_grad(H, a, h->grad_ws, partials, (double*)out[6], h->ws_words + 1, s);
                          },
                          x);
    });
}

// The forward mode of the exact compact solve: one launch, one lane per (direction, instance), of the tangent sweep on
// the model and the model's tangent built from v and the direction (mpc_compact_tangent.hip).  One entry for both
// parameter modes, as tpc_mpc_solve_batch_compact_exact_from takes an optional params_rows; a one-launch entry like the
// general forward pass (staged_run), the shared parameters' tangent a row of K * 10 elements.
int tpc_mpc_solve_batch_compact_exact_forward(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                              const void* delta_y, const void* delta_phi, const void* params_rows,
                                              const void* sequence, const int32_t* status,
                                              const tpc_mpc_compact_tangents* t, void* tfront, void* trear,
                                              void* tsequence, uint32_t* flags_out, int mem, void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_solve_batch_compact_exact_forward");
        const bool rows = params_rows != nullptr;
        if (!rows) {
            rc = check_compact_model(h, p);
            if (rc) return rc;
        }
        rc = check_batch(h, n, mem);
        if (rc) return rc;
        if (!t) return fail(h, TPC_MPC_ERR_BAD_ARG, "null tangent struct");
        if (t->directions < 1 || (int64_t)t->directions * n > 0x7fffffffll)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "need directions >= 1 and directions * n < 2^31");
        if (rows && t->tparams)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "tparams is the shared parameters' tangent: with params_rows give tparams_rows");
        if (!rows && t->tparams_rows) return fail(h, TPC_MPC_ERR_BAD_ARG, "tparams_rows needs params_rows");
        if (!tfront && !trear && !tsequence) return fail(h, TPC_MPC_ERR_BAD_ARG, "no output asked for");
        rc = check_host_only_pass(h, mem, "forward pass");
        if (rc) return rc;
        if (n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        if (!v || !delta_y || !delta_phi) return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
        if (!sequence) return fail(h, TPC_MPC_ERR_BAD_ARG, "null sequence");
        const int H = p->horizon, K = t->directions;
        constexpr int kP = ctan::kParams;
        const bool whole = tsequence != nullptr;
        // the arrays in order: 11 inputs (params_rows, status -- int32 -- and every tangent may be null), then 3
        // outputs; tparams is one row of K * kP elements, not one element per instance
        const void* src[11] = {params_rows, v, delta_y, delta_phi, sequence, status, t->tv, t->tdelta_y, t->tdelta_phi,
                               t->tparams, t->tparams_rows};
        void* dst[3] = {tfront, trear, tsequence};
        const int64_t comps[14] = {kP, 1, 1, 1, 2 * H, 1, K, K, K, 1, (int64_t)K * kP, K, K, (int64_t)K * 2 * H};
        int width[14] = {0};
        width[5] = 4;
        int64_t elems[14] = {0};
        elems[9] = (int64_t)K * kP;
        StagedExtra x;
        x.width = width;
        x.elems = elems;
        return staged_run(h, n, n, mem, stream, flags_out, compact_tangent_scratch_bytes(H, n, K, whole), src, dst, comps,
                          [&](int64_t ld, const void* const* in, void* const* out, hipStream_t s, uint32_t* hf) {
                              ctan::Args a;
                              std::memset(&a, 0, sizeof(a));
                              a.n = n; a.ld = ld; a.K = K;
                              if (!rows) bind_compact_model(&a, p);
                              a.params = (const double*)in[0];
                              a.v = (const double*)in[1]; a.dy = (const double*)in[2]; a.dphi = (const double*)in[3];
                              a.seq = (const double*)in[4]; a.status = (const int32_t*)in[5];
                              a.tv = (const double*)in[6]; a.tdy = (const double*)in[7]; a.tdphi = (const double*)in[8];
                              a.tparams = (const double*)in[9]; a.tparams_rows = (const double*)in[10];
                              a.tfront = (double*)out[0]; a.trear = (double*)out[1]; a.tseq = (double*)out[2];
                              if (hf) { *hf = compact_tangent_host(H, a); return hipSuccess; }
                              return compact_tangent(H, a, h->grad_ws, h->ws_words + 1, s);
                          },
                          x);
    });
}

// what the three plant entries check of a tpc_mpc_plant (after check_common and check_general_io)
static int check_plant(tpc_mpc_context* h, const tpc_mpc_general_io* io, const tpc_mpc_plant* plant) {
    if (!plant) return fail(h, TPC_MPC_ERR_BAD_ARG, "null plant struct");
    const int given = (plant->A ? 1 : 0) + (plant->B ? 1 : 0) + (plant->C ? 1 : 0);
    if (given != 0 && given != 3)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "the plant's A, B, C: all three or none");
    if (plant->disturbance && plant->ld_d < io->n)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "the disturbance needs ld_d >= n");
    return TPC_MPC_OK;
}

int tpc_mpc_rollout_plant(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                          const tpc_mpc_plant* plant, int32_t loop, int32_t steps, const void* new_last_targets,
                          const tpc_mpc_polish* q, int32_t fallback, void* controls_out, void* states_out,
                          int32_t* iters_out, void* sequences_out, int32_t* first_unverified, uint32_t* flags_out,
                          int mem, void* stream) {
    int rc = guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_rollout_plant");
        rc = check_general_io(h, io, mem);
        if (rc) return rc;
        rc = check_plant(h, io, plant);
        if (rc) return rc;
        if (loop != TPC_MPC_LOOP_RECORD && loop != TPC_MPC_LOOP_POLISHED && loop != TPC_MPC_LOOP_NEWTON)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "unknown loop %d", (int)loop);
        return TPC_MPC_OK;
    });
    if (rc) return rc;
    if (loop == TPC_MPC_LOOP_NEWTON)
        return rollout_newton_impl(h, p, io, steps, new_last_targets, q, fallback, controls_out, states_out, iters_out,
                                   sequences_out, first_unverified, flags_out, mem, stream, plant);
    const bool polished = loop == TPC_MPC_LOOP_POLISHED;
    return rollout_impl(h, p, io, steps, new_last_targets, controls_out, states_out, iters_out, sequences_out, !polished,
                        polished, polished ? q : nullptr, flags_out, mem, stream, plant);
}

// tpc_mpc_rollout_backward (plant and pg null) and tpc_mpc_rollout_plant_backward (both given, the plant checked below)
static int rollout_backward_impl(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, int32_t steps,
                                 const void* new_last_targets, const tpc_mpc_rollout_grad* g, uint32_t* flags_out,
                                 int mem, void* stream, const char* name, bool with_plant, const tpc_mpc_plant* plant,
                                 const tpc_mpc_plant_grad* pg) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, name);
        rc = check_general_io(h, io, mem);
        if (rc) return rc;
        if (!g) return fail(h, TPC_MPC_ERR_BAD_ARG, "null gradient struct");
        if (with_plant) {
            rc = check_plant(h, io, plant);
            if (rc) return rc;
            if (!pg) return fail(h, TPC_MPC_ERR_BAD_ARG, "null plant gradient struct");
            if (!plant->A && (pg->dA || pg->dB || pg->dC))
                return fail(h, TPC_MPC_ERR_BAD_ARG, "the plant's dA, dB, dC asked for without the plant's A, B, C");
            if (pg->ddisturbance && plant->ld_d != 0 && plant->ld_d < io->n)
                return fail(h, TPC_MPC_ERR_BAD_ARG, "ddisturbance needs ld_d >= n (or 0: the io's ld)");
        }
        rc = check_steps(h, steps);
        if (rc) return rc;
        if (g->dnew_last_targets && !new_last_targets)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "dnew_last_targets asked for without new_last_targets");
        rc = check_host_only_pass(h, mem, "backward pass");
        if (rc) return rc;
        if (io->n == 0 || steps == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        rc = check_model(h, io);
        if (rc) return rc;
        if (!g->sequences || !g->states) return fail(h, TPC_MPC_ERR_BAD_ARG, "null sequences / states");
        const int I = io->inputs, H = p->horizon;
        const int64_t n = io->n, S = steps;
        // the plant kernel runs when the plant changes anything: its own arrays, or the disturbance's gradient
        const bool sep = with_plant && plant->A, use_plant = sep || (with_plant && pg->ddisturbance);
        const int64_t ld_dd = with_plant && plant->ld_d ? plant->ld_d : io->ld;   // of ddisturbance, in the caller's memory
        // the io's, g's and the plant's arrays in order: 17 inputs (the optional ones may be null), then 15 outputs,
        // with their component counts
        constexpr int kIn = 17, kOut = 15;
        const void* src[kIn] = {io->A, io->B, io->C, io->Q, io->R, io->lower, io->upper, io->x0, io->targets,
                                new_last_targets, g->sequences, g->states, g->grad_controls, g->grad_states,
                                sep ? plant->A : nullptr, sep ? plant->B : nullptr, sep ? plant->C : nullptr};
        void* dst[kOut] = {g->dA, g->dB, g->dC, g->dQ, g->dR, g->dlower, g->dupper, g->dx0, g->dtargets,
                           g->dnew_last_targets, g->kkt_residual, sep ? pg->dA : nullptr, sep ? pg->dB : nullptr,
                           sep ? pg->dC : nullptr, use_plant ? pg->ddisturbance : nullptr};
        const int64_t rows[kIn + kOut] = {4, 2 * I, 2, 2, I, I, I, 2, 2 * H, 2 * S, S * H * I, 2 * S, S * I, 2 * S,
                                          4, 2 * I, 2,
                                          4, 2 * I, 2, 2, I, I, I, 2, 2 * H, 2 * S, 1, 4, 2 * I, 2, 2 * S};
        int64_t lds[kIn + kOut] = {0};
        lds[kIn + 14] = ld_dd;
        StagedExtra x;
        x.ld = lds;
        const bool staged = !h->host_only && mem == TPC_MPC_HOST;
        return staged_run(h, n, io->ld, mem, stream, flags_out, grad_scratch_bytes(I, H, n), src, dst, rows,
                          [&](int64_t ld, const void* const* in, void* const* out, hipStream_t s, uint32_t* hf) {
                              grad::RollArgs a;
                              std::memset(&a, 0, sizeof(a));
                              a.n = n; a.ld = ld; a.steps = steps;
                              bind_model(&a, in);
                              a.nlt = (const double*)in[9]; a.seq = (const double*)in[10];
                              a.states = (const double*)in[11]; a.gu = (const double*)in[12];
                              a.gx = (const double*)in[13];
                              a.dA = (double*)out[0]; a.dB = (double*)out[1]; a.dC = (double*)out[2];
                              a.dQ = (double*)out[3]; a.dR = (double*)out[4]; a.dlo = (double*)out[5];
                              a.dhi = (double*)out[6]; a.dx0 = (double*)out[7]; a.dtargets = (double*)out[8];
                              a.dnlt = (double*)out[9]; a.kkt = (double*)out[10];
                              if (!use_plant) {
                                  if (hf) { *hf = rollout_grad_host(I, H, a); return hipSuccess; }
                                  return rollout_grad(I, H, a, h->grad_ws, h->ws_words + 1, s);
                              }
                              grad::RollPlant pl;
                              std::memset(&pl, 0, sizeof(pl));
                              pl.separate = sep ? 1 : 0;
                              pl.A = sep ? (const double*)in[14] : a.A; pl.B = sep ? (const double*)in[15] : a.B;
                              pl.C = sep ? (const double*)in[16] : a.C;
                              pl.dA = (double*)out[11]; pl.dB = (double*)out[12]; pl.dC = (double*)out[13];
                              pl.dd = (double*)out[14];
                              pl.ld_d = staged ? ld : ld_dd;
                              if (hf) { *hf = rollout_plant_grad_host(I, H, a, pl); return hipSuccess; }
                              return rollout_plant_grad(I, H, a, pl, h->grad_ws, h->ws_words + 1, s);
                          },
                          x);
    });
}

int tpc_mpc_rollout_backward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, int32_t steps,
                             const void* new_last_targets, const tpc_mpc_rollout_grad* g, uint32_t* flags_out,
                             int mem, void* stream) {
    return rollout_backward_impl(h, p, io, steps, new_last_targets, g, flags_out, mem, stream,
                                 "tpc_mpc_rollout_backward", false, nullptr, nullptr);
}

int tpc_mpc_rollout_plant_backward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                   const tpc_mpc_plant* plant, int32_t steps, const void* new_last_targets,
                                   const tpc_mpc_rollout_grad* g, const tpc_mpc_plant_grad* pg, uint32_t* flags_out,
                                   int mem, void* stream) {
    return rollout_backward_impl(h, p, io, steps, new_last_targets, g, flags_out, mem, stream,
                                 "tpc_mpc_rollout_plant_backward", true, plant, pg);
}

int tpc_mpc_solve_batch_general_forward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                        const void* controls, const tpc_mpc_tangents* t, void* tcontrols,
                                        uint32_t* flags_out, int mem, void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, "tpc_mpc_solve_batch_general_forward");
        rc = check_general_io(h, io, mem);
        if (rc) return rc;
        if (!t) return fail(h, TPC_MPC_ERR_BAD_ARG, "null tangent struct");
        if (t->directions < 1 || (int64_t)t->directions * io->n > 0x7fffffffll)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "need directions >= 1 and directions * n < 2^31");
        rc = check_host_only_pass(h, mem, "forward pass");
        if (rc) return rc;
        if (io->n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        rc = check_model(h, io);
        if (rc) return rc;
        if (!controls || !tcontrols) return fail(h, TPC_MPC_ERR_BAD_ARG, "null controls / tcontrols");
        const int I = io->inputs, H = p->horizon, K = t->directions;
        const int64_t n = io->n;
        // ten primal inputs, ten tangents (K stacked blocks each; tnew_last_targets is not used here), one output
        const void* src[20] = {io->A, io->B, io->C, io->Q, io->R, io->lower, io->upper, io->x0, io->targets, controls,
                               t->tA, t->tB, t->tC, t->tQ, t->tR, t->tlower, t->tupper, t->tx0, t->ttargets, nullptr};
        void* dst[1] = {tcontrols};
        const int64_t rows[21] = {4, 2 * I, 2, 2, I, I, I, 2, 2 * H, H * I,
                                  4 * K, 2 * I * K, 2 * K, 2 * K, I * K, I * K, I * K, 2 * K, 2 * H * K, 0,
                                  (int64_t)H * I * K};
        return staged_run(h, n, io->ld, mem, stream, flags_out, tangent_scratch_bytes(I, H, n, K, true), src, dst, rows,
                          [&](int64_t ld, const void* const* in, void* const* out, hipStream_t s, uint32_t* hf) {
                              tangent::Args a;
                              std::memset(&a, 0, sizeof(a));
                              a.n = n; a.ld = ld; a.K = K;
                              bind_model(&a, in);
                              a.u = (const double*)in[9];
                              a.t = bind_dirs(in + 10);
                              a.tu = (double*)out[0];
                              if (hf) { *hf = tangent_general_host(I, H, a); return hipSuccess; }
                              return tangent_general(I, H, a, h->grad_ws, h->ws_words + 1, s);
                          });
    });
}

// tpc_mpc_rollout_forward (with_plant false) and tpc_mpc_rollout_plant_forward
static int rollout_forward_impl(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, int32_t steps,
                                const void* new_last_targets, const void* sequences, const void* states,
                                const tpc_mpc_tangents* t, void* tcontrols, void* tstates, uint32_t* flags_out, int mem,
                                void* stream, const char* name, bool with_plant, const tpc_mpc_plant* plant,
                                const tpc_mpc_plant_tangents* pt) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p, true);
        if (rc) return rc;
        if (p->dtype != TPC_MPC_F64) return fp64_only(h, name);
        rc = check_general_io(h, io, mem);
        if (rc) return rc;
        if (!t) return fail(h, TPC_MPC_ERR_BAD_ARG, "null tangent struct");
        tpc_mpc_plant_tangents none;
        std::memset(&none, 0, sizeof(none));
        if (with_plant) {
            rc = check_plant(h, io, plant);
            if (rc) return rc;
            if (!pt) pt = &none;
            if (!plant->A && (pt->tA || pt->tB || pt->tC))
                return fail(h, TPC_MPC_ERR_BAD_ARG, "the plant's tA, tB, tC given without the plant's A, B, C");
            if (pt->tdisturbance && plant->ld_d != 0 && plant->ld_d < io->n)
                return fail(h, TPC_MPC_ERR_BAD_ARG, "tdisturbance needs ld_d >= n (or 0: the io's ld)");
        }
        rc = check_steps(h, steps);
        if (rc) return rc;
        if (t->directions < 1 || (int64_t)t->directions * io->n > 0x7fffffffll)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "need directions >= 1 and directions * n < 2^31");
        if (t->tnew_last_targets && !new_last_targets)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "tnew_last_targets given without new_last_targets");
        rc = check_host_only_pass(h, mem, "forward pass");
        if (rc) return rc;
        if (io->n == 0 || steps == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        rc = check_model(h, io);
        if (rc) return rc;
        if (!sequences || !states || !tcontrols) return fail(h, TPC_MPC_ERR_BAD_ARG, "null sequences / states / tcontrols");
        const int I = io->inputs, H = p->horizon, K = t->directions;
        const int64_t n = io->n, S = steps;
        // the plant kernel runs when the plant changes anything: its own arrays, or the disturbance's tangent
        const bool sep = with_plant && plant->A, use_plant = sep || (with_plant && pt->tdisturbance);
        const int64_t ld_td = with_plant && plant->ld_d ? plant->ld_d : io->ld;   // of tdisturbance, in the caller's memory
        const bool staged = !h->host_only && mem == TPC_MPC_HOST;
        // twelve primal inputs (new_last_targets may be null), ten tangents (K stacked blocks each), the plant's three
        // arrays, three tangents and the disturbance's tangent; two outputs
        constexpr int kIn = 29;
        const void* src[kIn] = {io->A, io->B, io->C, io->Q, io->R, io->lower, io->upper, io->x0, io->targets,
                                new_last_targets, sequences, states,
                                t->tA, t->tB, t->tC, t->tQ, t->tR, t->tlower, t->tupper, t->tx0, t->ttargets,
                                t->tnew_last_targets,
                                sep ? plant->A : nullptr, sep ? plant->B : nullptr, sep ? plant->C : nullptr,
                                sep ? pt->tA : nullptr, sep ? pt->tB : nullptr, sep ? pt->tC : nullptr,
                                use_plant ? pt->tdisturbance : nullptr};
        int64_t lds[kIn + 2] = {0};
        lds[28] = ld_td;
        void* dst[2] = {tcontrols, tstates};
        const int64_t rows[kIn + 2] = {4, 2 * I, 2, 2, I, I, I, 2, 2 * H, 2 * S, S * H * I, 2 * S,
                                       4 * K, 2 * I * K, 2 * K, 2 * K, I * K, I * K, I * K, 2 * K, 2 * H * K, 2 * S * K,
                                       4, 2 * I, 2, 4 * K, 2 * I * K, 2 * K, 2 * S * K,
                                       S * I * K, 2 * S * K};
        StagedExtra x;
        x.ld = lds;
        return staged_run(h, n, io->ld, mem, stream, flags_out, tangent_scratch_bytes(I, H, n, K, false), src, dst, rows,
                          [&](int64_t ld, const void* const* in, void* const* out, hipStream_t s, uint32_t* hf) {
                              tangent::RollArgs a;
                              std::memset(&a, 0, sizeof(a));
                              a.n = n; a.ld = ld; a.steps = steps; a.K = K;
                              bind_model(&a, in);
                              a.nlt = (const double*)in[9]; a.seq = (const double*)in[10];
                              a.states = (const double*)in[11];
                              a.t = bind_dirs(in + 12);
                              a.tu = (double*)out[0]; a.tx = (double*)out[1];
                              if (!use_plant) {
                                  if (hf) { *hf = rollout_tangent_host(I, H, a); return hipSuccess; }
                                  return rollout_tangent(I, H, a, h->grad_ws, h->ws_words + 1, s);
                              }
                              tangent::RollPlant pl;
                              std::memset(&pl, 0, sizeof(pl));
                              pl.A = sep ? (const double*)in[22] : a.A; pl.B = sep ? (const double*)in[23] : a.B;
                              pl.C = sep ? (const double*)in[24] : a.C;
                              pl.tA = sep ? (const double*)in[25] : a.t.tA; pl.tB = sep ? (const double*)in[26] : a.t.tB;
                              pl.tC = sep ? (const double*)in[27] : a.t.tC;
                              pl.td = (const double*)in[28];
                              pl.ld_d = staged ? ld : ld_td;
                              if (hf) { *hf = rollout_plant_tangent_host(I, H, a, pl); return hipSuccess; }
                              return rollout_plant_tangent(I, H, a, pl, h->grad_ws, h->ws_words + 1, s);
                          },
                          x);
    });
}

int tpc_mpc_rollout_forward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, int32_t steps,
                            const void* new_last_targets, const void* sequences, const void* states,
                            const tpc_mpc_tangents* t, void* tcontrols, void* tstates, uint32_t* flags_out, int mem,
                            void* stream) {
    return rollout_forward_impl(h, p, io, steps, new_last_targets, sequences, states, t, tcontrols, tstates, flags_out,
                                mem, stream, "tpc_mpc_rollout_forward", false, nullptr, nullptr);
}

int tpc_mpc_rollout_plant_forward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                  const tpc_mpc_plant* plant, int32_t steps, const void* new_last_targets,
                                  const void* sequences, const void* states, const tpc_mpc_tangents* t,
                                  const tpc_mpc_plant_tangents* pt, void* tcontrols, void* tstates,
                                  uint32_t* flags_out, int mem, void* stream) {
    return rollout_forward_impl(h, p, io, steps, new_last_targets, sequences, states, t, tcontrols, tstates, flags_out,
                                mem, stream, "tpc_mpc_rollout_plant_forward", true, plant, pt);
}

namespace {

int check_trajectories(tpc_mpc_context* h, const tpc_mpc_params* p, const tpc_mpc_trajectories* t,
                       const float* lookup_x, const float* lookup_y, int32_t lookup_n) {
    if (p->dtype != TPC_MPC_F64) return fail(h, TPC_MPC_ERR_BAD_ARG, "follow_batch solves in fp64");
    if (!t) return fail(h, TPC_MPC_ERR_BAD_ARG, "null trajectories");
    if (t->n < 0 || t->ld < t->n || t->n > 0x7fffffffll || t->max_points < 0 || lookup_n < 0)
        return fail(h, TPC_MPC_ERR_BAD_ARG, "need 0 <= n <= ld, n < 2^31, max_points >= 0, lookup_n >= 0");
    if (t->n == 0) return TPC_MPC_OK;
    if (!t->pos_x || !t->pos_y || !t->dir_x || !t->dir_y || !t->velocity || !t->count || !t->car_velocity ||
        !t->look_ahead || (lookup_n > 0 && (!lookup_x || !lookup_y)))
        return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
    return TPC_MPC_OK;
}

FollowArgs follow_args(const tpc_mpc_trajectories* t, const float* lookup_x, const float* lookup_y, int32_t lookup_n) {
    FollowArgs fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.n = t->n; fa.ld = t->ld; fa.max_points = t->max_points;
    fa.px = t->pos_x; fa.py = t->pos_y; fa.dx = t->dir_x; fa.dy = t->dir_y; fa.vel = t->velocity;
    fa.count = t->count; fa.car_velocity = t->car_velocity; fa.look_ahead = t->look_ahead;
    fa.lut_x = lookup_x; fa.lut_y = lookup_y; fa.lut_n = lookup_n;
    return fa;
}

}  // namespace

int tpc_mpc_follow_batch(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_trajectories* t,
                         const float* lookup_x, const float* lookup_y, int32_t lookup_n,
                         double* steering_front, double* steering_rear, float* target_speed,
                         float* target_distance, int32_t* iters, uint32_t* flags_out, void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p);
        if (rc) return rc;
        rc = check_compact_model(h, p);
        if (rc) return rc;
        rc = check_trajectories(h, p, t, lookup_x, lookup_y, lookup_n);
        if (rc) return rc;
        if (t->n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        if (!steering_front || !steering_rear || !target_speed || !target_distance)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        const int64_t n = t->n;
        StreamOrderScope order(h, s);
        rc = order.begin();
        if (rc) return rc;
        // v | y_soll | phi_soll (the compact solve's inputs), produced on device
        const int64_t col = pad256(n * 8);
        rc = ensure(h, &h->roll, &h->roll_bytes, 3 * col);
        if (rc) return rc;
        char* b = (char*)h->roll;
        FollowArgs fa = follow_args(t, lookup_x, lookup_y, lookup_n);
        fa.v_out = (double*)b; fa.ysoll_out = (double*)(b + col); fa.phisoll_out = (double*)(b + 2 * col);
        fa.target_speed = target_speed; fa.target_distance = target_distance;
        hipError_t e = launch_traj_point(fa, s);
        if (e != hipSuccess) return hip_fail(h, e, "traj_point launch");
        HIP_TRY(h, hipMemsetAsync(h->ws_words + 1, 0, sizeof(uint32_t), s));
        rc = compact_launch(h, p, n, fa.v_out, fa.ysoll_out, fa.phisoll_out, steering_front, steering_rear, iters, s);
        if (rc) return rc;
        e = launch_follow_post(n, target_speed, steering_front, steering_rear, s);
        if (e != hipSuccess) return hip_fail(h, e, "follow_post launch");
        rc = order.end();
        if (rc) return rc;
        return finish_flags(h, flags_out, s);
    });
}

int tpc_mpc_follow_batch_horizon(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_trajectories* t,
                                 const float* step_spacing, const float* lookup_x, const float* lookup_y,
                                 int32_t lookup_n, double* steering_front, double* steering_rear,
                                 float* target_speed, float* target_distance, double* targets_out,
                                 int32_t* iters, uint32_t* flags_out, void* stream) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p);
        if (rc) return rc;
        rc = check_compact_model(h, p);
        if (rc) return rc;
        rc = check_trajectories(h, p, t, lookup_x, lookup_y, lookup_n);
        if (rc) return rc;
        if (t->n == 0) { if (flags_out) *flags_out = 0; return TPC_MPC_OK; }
        if (!steering_front || !steering_rear || !target_speed || !target_distance)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "null batch pointer");
        HIP_TRY(h, hipSetDevice(h->device));
        hipStream_t s = (hipStream_t)stream;
        const int64_t n = t->n;
        const int H = p->horizon, I = 2;
        const int algo = pick_algo(h, p->algo, I, H, n, p->dtype, fma_general_usable(H, nullptr, nullptr), false, group_general_usable(p->dtype, H, nullptr, nullptr));
        if (algo < 0) return fail(h, TPC_MPC_ERR_BAD_HORIZON, "the WAVE kernel exists for the specialised horizons with inputs*horizon <= 64 only; use LANE or AUTO");
        StreamOrderScope order(h, s);
        rc = order.begin();
        if (rc) return rc;
        // general-form batch built on device: A[4] B[4] C[2] Q[2] R[2] lo[2] hi[2] x0[2] targets[2H] u0[2]
        const int64_t ldw = (n + 63) / 64 * 64;
        const int comps[10] = {4, 4, 2, 2, 2, 2, 2, 2, 2 * H, 2};
        int64_t off[10], total = 0;
        for (int c = 0; c < 10; ++c) { off[c] = total; total += pad256((int64_t)comps[c] * ldw * 8); }
        rc = ensure(h, &h->roll, &h->roll_bytes, total);
        if (rc) return rc;
        char* w = (char*)h->roll;
        FollowArgs fa = follow_args(t, lookup_x, lookup_y, lookup_n);
        fa.target_speed = target_speed; fa.target_distance = target_distance;
        FollowHorizonArgs fh;
        std::memset(&fh, 0, sizeof(fh));
        fh.H = H; fh.ldw = ldw; fh.step_spacing = step_spacing;
        fh.step = p->step_size; fh.wheelbase = p->wheelbase;
        fh.q[0] = p->weight_y; fh.q[1] = p->weight_phi;
        fh.r[0] = p->weight_steering_front; fh.r[1] = p->weight_steering_rear;
        for (int j = 0; j < 2; ++j) { fh.lo[j] = p->lower[j]; fh.hi[j] = p->upper[j]; }
        fh.A = (double*)(w + off[0]); fh.B = (double*)(w + off[1]); fh.C = (double*)(w + off[2]);
        fh.Q = (double*)(w + off[3]); fh.R = (double*)(w + off[4]); fh.lo_out = (double*)(w + off[5]);
        fh.hi_out = (double*)(w + off[6]); fh.x0 = (double*)(w + off[7]); fh.targets = (double*)(w + off[8]);
        fh.targets_copy = targets_out; fh.ld_copy = n;
        hipError_t e = launch_traj_horizon(fa, fh, s);
        if (e != hipSuccess) return hip_fail(h, e, "traj_horizon launch");

        GeneralArgs a;
        std::memset(&a, 0, sizeof(a));
        a.n = n; a.ld = ldw; a.shift_controls = 1;
        a.A = fh.A; a.B = fh.B; a.C = fh.C; a.Q = fh.Q; a.R = fh.R; a.lo = fh.lo_out; a.hi = fh.hi_out;
        a.x0 = fh.x0; a.targets = fh.targets; a.u0 = w + off[9]; a.iters = iters;
        a.flags = h->ws_words + 1;
        const bool fix = wants_cap_resolve(p, algo);
        if (fix && !a.iters) {
            rc = cap_iters_buffer(h, n, &a.iters);
            if (rc) return rc;
        }
        if (fix) {
            rc = resolve_reserve(h, H, TPC_MPC_F64, n);
            if (rc) return rc;
        }
        Workspace ws;
        rc = prepare_workspace(h, algo, H, TPC_MPC_F64, n, &ws, 1);
        if (rc) return rc;
        HIP_TRY(h, hipMemsetAsync(h->ws_words + 1, 0, sizeof(uint32_t), s));
        e = dispatch_general(algo, I, H, TPC_MPC_F64, a, knobs_of(p), ws, s);
        if (e == hipSuccess && fix) {
            Workspace ws2;
            rc = resolve_workspace(h, H, TPC_MPC_F64, n, &ws2);
            if (rc) return rc;
            e = resolve_general(I, H, a, knobs_of(p), ws2, s);
        }
        if (e != hipSuccess) return hip_fail(h, e, "kernel launch");
        // u0[2][ldw] -> (front, rear), then the crossing rule
        HIP_TRY(h, hipMemcpyAsync(steering_front, w + off[9], n * 8, hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(steering_rear, w + off[9] + ldw * 8, n * 8, hipMemcpyDeviceToDevice, s));
        e = launch_follow_post(n, target_speed, steering_front, steering_rear, s);
        if (e != hipSuccess) return hip_fail(h, e, "follow_post launch");
        rc = order.end();
        if (rc) return rc;
        return finish_flags(h, flags_out, s);
    });
}

int tpc_mpc_reserve(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, int mem) {
    return guarded(h, [&]() -> int {
        int rc = check_common(h, p);
        if (rc) return rc;
        rc = check_batch(h, n, mem);
        if (rc) return rc;
        if (n == 0) return TPC_MPC_OK;
        HIP_TRY(h, hipSetDevice(h->device));
        // the larger of the kernel families' needs, so that every choice of AUTO is covered -- and the buffer the
        // re-solve of capped instances reads its iteration counts from when the caller passes none
        rc = reserve_lane_workspace(h, p->horizon, p->dtype, n);
        if (rc) return rc;
        if (p->algo == TPC_MPC_ALGO_AUTO && p->dtype == TPC_MPC_F64) {
            int32_t* unused = nullptr;
            rc = cap_iters_buffer(h, n, &unused);
            if (rc) return rc;
            // AUTO's presolve: its scratch, side stream and events (sized as presolve_begin / general_launch size them
            // for two inputs and ld = n)
            Presolve ps;
            if (presolve_lambda(p) > 0.0 && presolve_share(h, n, &ps)) {
                Workspace unused_ws;
                char* side = nullptr;
                rc = presolve_scratch(h, p->horizon, p->dtype, n, 2 * pad256(n * 8) + pad256(n * 4), &unused_ws, &side);
                if (rc) return rc;
            }
        }
        if (mem == TPC_MPC_HOST) {
            rc = ensure(h, &h->stage, &h->stage_bytes, compact_stage_bytes(p->dtype, n));
            if (rc) return rc;
        }
        return TPC_MPC_OK;
    });
}

int tpc_mpc_x_set_work_hint(tpc_mpc_handle h, const int32_t* hint, int64_t n, int mem) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (h->host_only) return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle");
        h->hint = nullptr;
        h->hint_n = 0;
        if (!hint || n == 0) return TPC_MPC_OK;   // cleared
        int rc = check_batch(h, n, mem);
        if (rc) return rc;
        // always the handle's own copy: no caller pointer outlives the call that received it
        HIP_TRY(h, hipSetDevice(h->device));
        rc = ensure(h, &h->hint_own, &h->hint_own_bytes, n * 4);
        if (rc) return rc;
        // the previous solve may still be reading the old copy: wait for it (its stream-order event), then copy
        // synchronously -- a DEVICE hint must be complete when this is called
        if (h->have_last) HIP_TRY(h, hipEventSynchronize(h->done_ev));
        HIP_TRY(h, hipMemcpy(h->hint_own, hint, (size_t)n * 4,
                             mem == TPC_MPC_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
        h->hint = (const int32_t*)h->hint_own;
        h->hint_n = n;
        return TPC_MPC_OK;
    });
}

int tpc_mpc_x_set_queue_key(tpc_mpc_handle h, int on) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (on != 0 && on != 1) return fail(h, TPC_MPC_ERR_BAD_ARG, "tpc_mpc_x_set_queue_key takes 0 or 1");
        h->opt_queue_key = on != 0;
        return TPC_MPC_OK;
    });
}

int tpc_mpc_x_last_queue_key(tpc_mpc_handle h, int* key) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (!key) return fail(h, TPC_MPC_ERR_BAD_ARG, "null key");
        *key = h->last_queue_key;
        return TPC_MPC_OK;
    });
}

int tpc_mpc_x_set_group_share(tpc_mpc_handle h, int waves, int cu_count) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (waves < 0 || cu_count < 0) return fail(h, TPC_MPC_ERR_BAD_ARG, "need waves >= 0, cu_count >= 0");
        h->max_waves = waves;
        h->cu_count = cu_count > 0 ? cu_count : h->device_cu_count;   // (0: back to the device's own)
        return TPC_MPC_OK;
    });
}

int tpc_mpc_x_set_lanex_below(tpc_mpc_handle h, int64_t below) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (below < -1) return fail(h, TPC_MPC_ERR_BAD_ARG, "need below >= -1");
        h->opt_lanex_below = below;
        return TPC_MPC_OK;
    });
}

int tpc_mpc_set_option(tpc_mpc_handle h, int option, int64_t value) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        switch (option) {
            case TPC_MPC_OPT_WAVE_GROUP:
                if (value != 0 && value != 1 && value != 2 && value != 4)
                    return fail(h, TPC_MPC_ERR_BAD_ARG, "TPC_MPC_OPT_WAVE_GROUP takes 0, 1, 2 or 4");
                h->opt_wave_group = (int)value;
                return TPC_MPC_OK;
            case TPC_MPC_OPT_GROUP_LANES:
                if (value != 0 && value != 2 && value != 4 && value != 8)
                    return fail(h, TPC_MPC_ERR_BAD_ARG, "TPC_MPC_OPT_GROUP_LANES takes 0, 2, 4 or 8");
                h->opt_group_lanes = (int)value;
                return TPC_MPC_OK;
            case TPC_MPC_OPT_HOST_SOLVE_ONE:
                if (value < 0 || value > kMaxHorizon) return fail(h, TPC_MPC_ERR_BAD_ARG, "TPC_MPC_OPT_HOST_SOLVE_ONE takes a horizon, 0 .. 64");
                h->opt_host_horizon = (int)value;
                return TPC_MPC_OK;
            case TPC_MPC_OPT_MAILBOX_HOST:
                if (h->host_only) return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle");
                HIP_TRY(h, hipSetDevice(h->device));
                one_shot_destroy(h);   // the next solve_one sets its mailbox up again, where this option says
                h->opt_mailbox_host = value != 0;
                return TPC_MPC_OK;
        }
        return fail(h, TPC_MPC_ERR_BAD_ARG, "unknown option %d", option);
    });
}

int tpc_mpc_set_profiling(tpc_mpc_handle h, int enable) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (h->host_only) return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle");
        HIP_TRY(h, hipSetDevice(h->device));
        if (enable)
            for (auto& e : h->ev) if (!e) HIP_TRY(h, hipEventCreate(&e));
        h->profiling = enable != 0;
        h->ev_valid = false;
        return TPC_MPC_OK;
    });
}

int tpc_mpc_last_kernel_times(tpc_mpc_handle h, double* first_ms, double* second_ms, int* algo) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (!h->ev_valid)
            return fail(h, TPC_MPC_ERR_BAD_ARG, h->last_algo == kAlgoMixed ? "the last solve was a mixed-horizon batch: its bins ran on child handles"
                                                                            : "no profiled solve on this handle yet");
        HIP_TRY(h, hipEventSynchronize(h->ev[2]));
        float a = 0, b = 0;
        HIP_TRY(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
        HIP_TRY(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
        if (first_ms) *first_ms = a;
        if (second_ms) *second_ms = b;
        if (algo) *algo = h->last_algo;
        return TPC_MPC_OK;
    });
}

int tpc_mpc_last_lane_stats(tpc_mpc_handle h, uint64_t* wave_iterations, uint64_t* refill_blocks) {
    return guarded(h, [&]() -> int {
        if (!h) return fail(nullptr, TPC_MPC_ERR_BAD_ARG, "null handle");
        if (h->host_only) return fail(h, TPC_MPC_ERR_NO_DEVICE, "host-only handle");
        if (h->last_algo == kAlgoMixed)
            return fail(h, TPC_MPC_ERR_BAD_ARG, "the last solve was a mixed-horizon batch: its bins ran on child handles");
        HIP_TRY(h, hipSetDevice(h->device));
        unsigned long long st[2] = {0, 0};
        // waits for the handle's last solve only (its stream-order event), not for the whole device
        if (h->have_last) HIP_TRY(h, hipEventSynchronize(h->done_ev));
        HIP_TRY(h, hipMemcpy(st, h->ws_words + 4, sizeof(st), hipMemcpyDeviceToHost));
        if (wave_iterations) *wave_iterations = st[0];
        if (refill_blocks) *refill_blocks = st[1];
        return TPC_MPC_OK;
    });
}

}  // extern "C"
