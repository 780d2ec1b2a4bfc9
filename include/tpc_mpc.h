/* tpc_mpc.h -- C ABI of the MI355X-native batched MPC-QP solver (libtpc_mpc.so).
 *
 * This is the drop-in boundary for ONE path of lms-org/trajectory_controller: the per-cycle
 * box-constrained MPC QP that TrajectoryPointController::mpcControllerTobi solves through
 * dlib::mpc<2,2,H>::operator().  Every entry point names the reference interface it replaces
 * (paths relative to the reference tree).  The library reproduces dlib's iteration sequence
 * (coordinate descent for `smo_iters` iterations, then accelerated projected gradient, stop when
 * the largest free gradient component is < eps), so in fp64 its outputs equal the reference's.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; no exception crosses this boundary.
 *   - every function returns a tpc_mpc_status (0 = ok); tpc_mpc_last_error() gives text.
 *   - the solve runs on the GPU.  There is no CPU fallback: without a usable gfx950 device
 *     tpc_mpc_create fails with TPC_MPC_ERR_NO_DEVICE.
 *   - a handle is not thread-safe; distinct handles are independent.  The library never keeps a
 *     caller pointer past the call that received it.
 *   - all solves of one handle share its device scratch and therefore never overlap: a solve
 *     submitted to a different stream than the handle's previous one first makes that stream wait
 *     for the previous solve (an event, no host synchronisation).  Batches that should run
 *     concurrently use one handle each.
 *   - batch arrays are structure-of-arrays: component c of instance k lives at base[c*ld + k]
 *     (`ld` >= n is the leading dimension, normally n; a shard of a larger batch passes the
 *     shard's base pointer and the full batch's ld).  Element type is `dtype` (double or float).
 */
#ifndef TPC_MPC_H
#define TPC_MPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPC_MPC_ABI_VERSION 5   /* 5 = 4 + new symbols only (the split-named sharded entries; later additions, such as
                                   tpc_mpc_solve_batch_general_backward, tpc_mpc_rollout_record / _backward / _polished / _newton, tpc_mpc_polish_batch_general
                                   and tpc_mpc_solve_batch_compact_exact / _exact_backward / _exact_rows / _exact_rows_backward / _exact_from / _exact_forward, are new symbols and structs only and keep 5);
                                   4 broke 3: tpc_mpc_params.reserved became .options and must be zero-initialised */

typedef struct tpc_mpc_context* tpc_mpc_handle;

typedef enum tpc_mpc_status {
    TPC_MPC_OK = 0,
    TPC_MPC_ERR_BAD_ARG = 1,        /* null pointer, n < 0, ld < n, unknown enum value          */
    TPC_MPC_ERR_BAD_WEIGHTS = 2,    /* min(Q) < 0 or min(R) <= 0   (mpc_abstract.h:90-97)       */
    TPC_MPC_ERR_BAD_BOUNDS = 3,     /* upper < lower               (mpc_abstract.h:90-97)       */
    TPC_MPC_ERR_BAD_HORIZON = 4,    /* horizon outside 1..64, or a kernel family that does not
                                       exist for it was demanded                                */
    TPC_MPC_ERR_BAD_EPS = 5,        /* eps <= 0                    (mpc.h:202 set_epsilon)      */
    TPC_MPC_ERR_NO_DEVICE = 6,      /* no gfx950 GPU / HIP runtime unusable                     */
    TPC_MPC_ERR_HIP = 7,            /* a HIP call failed; text in tpc_mpc_last_error            */
    TPC_MPC_ERR_ALLOC = 8,          /* host or device memory exhausted                          */
    TPC_MPC_ERR_COMM = 9            /* RCCL missing or an RCCL call failed (sharded solves)     */
} tpc_mpc_status;

typedef enum tpc_mpc_dtype { TPC_MPC_F64 = 0, TPC_MPC_F32 = 1 } tpc_mpc_dtype;

/* Where batch arrays live. */
typedef enum tpc_mpc_memory { TPC_MPC_HOST = 0, TPC_MPC_DEVICE = 1 } tpc_mpc_memory;

/* Kernel family.
 *   WAVE : one 64-lane wavefront per instance; lane j owns decision variable j and its row of the
 *          dense (I*H)x(I*H) Hessian (two variables per lane where I*H > 64: I = 2, H <= 64; the
 *          compact form at N = 40 instead builds its gradient from prefix sums over the lanes), the
 *          controls are exchanged by DPP / lane swaps, reductions by wavefront DPP/ballot.  (fp64
 *          batches of more than one instance per SIMD with I*H <= 32 run two instances per wavefront,
 *          one per 32-lane half, and four -- one per 16-lane row -- with I*H <= 16: same arithmetic per
 *          instance, every verdict per group; tpc_mpc_set_option(TPC_MPC_OPT_WAVE_GROUP, 1) keeps
 *          strictly one per wavefront.)  Lowest
 *          latency; used for small and mid-size batches and solve_one.  Needs a specialised horizon
 *          with I*H <= 64 or I = 2.  Agrees with the reference to ~1e-14 (same decisions, different
 *          summation).
 *   LANE : one lane per instance, dlib's O(H) recurrences unrolled in registers, 64 instances
 *          per wavefront with dynamic refill of finished lanes.  Bit-identical to the reference
 *          arithmetic in fp64; the bit-exact family for large batches.  fp64, N = 10, 20, 30, 40 (compact form, and the
 *          general form with or without controller state), batches
 *          that cannot fill the chip that way (below ~98 000 instances at N = 10 / 20, ~60 000 at N = 30 / 40): the
 *          projected-gradient phase runs G = N / 5 lanes per instance (csrc/mpc_lanex.h) -- dlib's two recurrences stay
 *          sequential, handed from lane to lane, everything else of an iteration is shared out; the same IEEE
 *          operations on the same operands, hence the same bits -- 16 384 instances of N = 40: 14.3 ms instead of 49.8,
 *          N = 20: 3.3 instead of 6.9.
 *   LANE_FMA : LANE's layout (one lane per instance, persistent wavefronts, refill queue) with the
 *          arithmetic rebuilt for the hardware instead of for dlib's rounding: controls in unit-box
 *          coordinates (dlib's clamp is the free [0,1] output clamp of the instruction that produces the
 *          value), fused multiply-adds, and the linear term folded into the backward recurrence (nothing
 *          of the model in memory): about half of LANE's instructions per iteration.  Same iteration and
 *          the same decisions as dlib on quantities that differ by rounding: max |du| vs dlib ~2e-13 at
 *          N = 20, ~1e-12 at N = 40, iteration counts identical on the BASELINE workloads.  They can differ
 *          in two cases only: where dlib's largest gradient component comes within rounding of eps, and where
 *          the coordinate-descent phase meets an arg-max that is a TIE in exact arithmetic -- dlib's strict '>'
 *          and this family's rounding then pick different components, both valid descent steps, and the two
 *          solves end at different points that both pass dlib's stop test.  Known: weight_phi <= 2^-30 weight_y
 *          (the heading is then costed through the position alone; N = 5 with step_size * v in -0.31 .. -0.21:
 *          2 % of a batch, |du| up to 1.3e-3).  Measured for WAVE too (7e-6); GROUP shares
 *          the arithmetic.  Compact form
 *          (solve_batch_compact, _mixed, _sharded) with hi > lo finite, specialised horizons.  General
 *          form (solve_batch_general without controls_inout / v_inout, follow_batch) at N = 4, 5, 10, 20:
 *          the same arithmetic in dlib's own coordinates (per-instance bounds may be pinned or infinite)
 *          with the linear term kept, scaled, as dlib keeps it: 1.2 - 1.5x LANE.  Requests it cannot
 *          take (controller state in or out, general form at N = 30 / 40, degenerate compact bounds, other
 *          horizons) run LANE.
 *   GROUP : G lanes per instance (2, 4 or 8; TPC_MPC_OPT_GROUP_LANES pins it), 64 / G instances per wavefront: the
 *          family between WAVE and LANE_FMA, for batches too large for a wavefront each and too small to give every
 *          lane of the chip an instance.  LANE_FMA's arithmetic with the horizon cut into G chunks: each lane runs
 *          its chunk's part of the two recurrences of mpc.h:275-281 in registers, and the chunks are joined by an
 *          exclusive scan over the lanes of the group (the recurrences are affine with a constant matrix, so joining
 *          costs log2 G steps of DPP moves and fused multiply-adds).  Persistent wavefronts, one per SIMD (fp32: two from
 *          the batch size at which that is faster -- a second resident wavefront nearly doubles a SIMD's fp32 issue rate
 *          and adds a tenth to its fp64 one), groups
 *          refilled from LANE_FMA's longest-first queue; the coordinate-descent phase and the records are LANE_FMA's
 *          own.  Compact form, N = 10, 20, 30, 40 (chunks padded where G does not divide N), the requests LANE_FMA
 *          takes; anything else runs LANE_FMA / LANE.  Same statement as LANE_FMA: max |du| vs dlib ~2e-13 at N = 20,
 *          ~1.5e-12 at N = 40, identical iteration counts.  16 384 instances of N = 20: 1.3 ms (WAVE 2.9, LANE_FMA
 *          3.5); of N = 40: 4.8 ms (15.0 / 30.6).
 *          General form (solve_batch_general, rollout, follow_batch*), fp64, N = 10, 20, 30, 40, one or two inputs:
 *          the chunks are joined by scans of 2x2 matrix powers (A is the instance's own: A^(L 2^s) computed once per
 *          refill), controller state in and out (controls_inout / v_inout) included -- behind the bit-exact
 *          coordinate-descent kernel there, and with dlib's own mask as the stop test, because a warm start may lie
 *          outside the box.  16 384 instances of N = 40, two inputs: 7.1 ms (WAVE 51, LANE 61).
 *   AUTO : the fastest family that meets the 1e-6 parity target, and it GUARANTEES that target where a guarantee is
 *          possible.  Family: WAVE below a crossover measured per dtype and horizon, then GROUP with 8, 4, 2 lanes
 *          per instance, then LANE_FMA (csrc/auto_table.h, generated by scripts/measure_crossover.py on a 256-CU
 *          part and scaled by the CU count: at N = 20 in fp64 WAVE below 7 094 instances, GROUP up to 160 530,
 *          LANE_FMA beyond -- in fp32 GROUP up to 321 060; at N = 30 and 40 GROUP is never overtaken, in either dtype and
 *          either form); LANE where none of them takes the request, and, in fp64, for every compact request with
 *          weight_phi <= 2^-30 weight_y and smo_iters > 0, whatever its size (solve_one included: one LANE launch
 *          instead of the resident wavefront) -- dlib's coordinate-descent arg-max can tie there (see LANE_FMA
 *          above), which no tolerance family follows to within 1e-6.  NOT covered: the general form
 *          (solve_batch_general, follow_batch_horizon, the rollouts) keeps its family when an instance's Q is
 *          (q0, ~0): the same tie can occur there and has not been measured or routed; ask for LANE.
 *          Guarantee (fp64, the specialised horizons,
 *          cold starts -- every compact entry point and the general form without controls_inout / v_inout): an
 *          instance that ends on max_iter has not converged, and over thousands of iterations of an ill-conditioned
 *          problem the tolerance families' rounding differences grow (2.3e-5 seen under adversarial parameters), so
 *          such instances are solved ONCE MORE by the bit-exact LANE kernels in the same call and come back with
 *          dlib's bits; every other instance took dlib's decisions on quantities that differ from dlib's by rounding
 *          (<= 1e-9 asserted, ~1e-12 observed).  The second pass costs three empty launches when nothing ended on
 *          the cap; when something did, it lasts max_iter bit-exact iterations (N = 10 / 20 / 30 / 40: G
 *          lanes per instance, 1.4 us per iteration at N = 40 -- 14 ms with dlib's cap of 10 000; BASELINE config 5,
 *          where a tenth of the N = 40 instances end there: 21.5 ms with it, 7 ms without; general form 2.1 us).
 *          A host that prefers the tolerance families' answer for capped instances sets TPC_MPC_PARAM_FAST_CAPPED in
 *          tpc_mpc_params.options; an explicitly demanded family is taken at its word; a host that needs dlib's bits
 *          everywhere asks for LANE. */
typedef enum tpc_mpc_algo {
    TPC_MPC_ALGO_AUTO = 0, TPC_MPC_ALGO_WAVE = 1, TPC_MPC_ALGO_LANE = 2, TPC_MPC_ALGO_LANE_FMA = 3, TPC_MPC_ALGO_GROUP = 4
} tpc_mpc_algo;

/* Non-fatal per-call flags, OR-ed into *flags_out (may be NULL). */
#define TPC_MPC_FLAG_NONFINITE 0x1u  /* an instance had NaN/Inf inputs: it returns the untouched
                                        start point like dlib does (every NaN comparison is
                                        false, mpc.h:298-311) and this flag is raised           */
#define TPC_MPC_FLAG_MAX_ITER  0x2u  /* an instance stopped on max_iter, not on eps             */
/*   (compact form, absurd speeds only -- |step_size * v| beyond 1e4 in fp32, 1e60 in fp64, where dlib's own
 *    intermediates overflow: dlib can stop early on an all-NaN gradient (its 0 * inf products) where these
 *    kernels keep +-inf and run to max_iter with the same controls; outputs agree, the iteration count and
 *    this flag may not.  DESIGN.md section 4.1.)                                                          */
#define TPC_MPC_FLAG_BAD_MODEL 0x4u  /* general form: an instance's Q, R or bounds break dlib's
                                        requires clause (mpc_abstract.h:90-97; min(Q) >= 0,
                                        min(R) > 0, upper >= lower).  dlib asserts (compiled out in
                                        the reference build); here the instance is not solved and
                                        returns its start point at iteration 0                    */

/* tpc_mpc_params.options */
#define TPC_MPC_PARAM_FAST_CAPPED 0x1  /* AUTO only: keep the tolerance family's answer for instances that end on
                                          max_iter instead of solving them once more bit-exactly (see AUTO above) */

/* Solver knobs.  Defaults (tpc_mpc_default_params) are dlib's and the reference module's:
 *   eps 0.01 (mpc.h:104), max_iter 10000 (mpc.h:103), smo_iters 50 (mpc.h:319),
 *   step_size 0.1 (src/trajectory_point_follower.cpp:96), wheelbase 0.21
 *   (include/trajectory_point_follower.h:47), weights 20/7/0.0005/10
 *   (src/trajectory_point_follower.cpp:92-95), bounds +-22 deg (src/...follower.cpp:16-18). */
typedef struct tpc_mpc_params {
    int32_t horizon;          /* H: MPC_HORIZON, include/trajectory_point_follower.h:48          */
    int32_t dtype;            /* tpc_mpc_dtype of the batch arrays and of the arithmetic          */
    int32_t algo;             /* tpc_mpc_algo                                                     */
    int32_t options;          /* TPC_MPC_PARAM_* bits, 0 by default                                */
    double eps;               /* dlib::mpc::set_epsilon        (mpc.h:197-208)                    */
    uint64_t max_iter;        /* dlib::mpc::set_max_iterations (mpc.h:190-195)                    */
    uint64_t smo_iters;       /* mpc.h:319                                                        */
    /* compact ("reference pattern") model, used by solve_one / solve_batch_compact only:         */
    double step_size;         /* mpcParameters.stepSize  T                                        */
    double wheelbase;         /* l                                                                */
    double weight_y, weight_phi, weight_steering_front, weight_steering_rear;
    double lower[2], upper[2];
} tpc_mpc_params;

/* ---- lifetime --------------------------------------------------------------------------------- */

/* Fill *p with the defaults above for horizon H, fp64, algo AUTO. */
int tpc_mpc_default_params(tpc_mpc_params* p, int horizon);

/* Create a solver bound to HIP device `device` (>= 0).  Owns device scratch; no other state.
 * device == TPC_MPC_DEVICE_NONE creates a HOST-ONLY handle: no GPU is looked for or touched, and the one call it serves
 * is tpc_mpc_solve_one -- on the calling thread, in the LANE_FMA family's arithmetic (csrc/tpc_mpc_host.cpp; fp64, the
 * specialised horizons, finite bounds with upper > lower, a CPU with fused multiply-add) -- which is what a host that
 * solves one short-horizon problem per cycle wants ("usable from any single thread without a GPU"): at
 * the reference's N = 4 a core needs ~3 us where the GPU round trip needs ~10.  The one other call it serves is
 * tpc_mpc_solve_batch_general_backward with TPC_MPC_HOST memory, also on the calling thread.  Every other batch entry
 * point returns TPC_MPC_ERR_NO_DEVICE on such a handle.  AUTO's re-solve of capped instances needs the GPU: a host-only handle
 * returns the tolerance answer and raises TPC_MPC_FLAG_MAX_ITER.  Likewise it has no bit-exact kernels for a request
 * with weight_phi <= 2^-30 weight_y: its answer there is the LANE_FMA family's, which can leave dlib's path at a tied arg-max (see
 * LANE_FMA above) and still passes dlib's stop test. */
#define TPC_MPC_DEVICE_NONE (-1)
int tpc_mpc_create(int device, tpc_mpc_handle* out);
int tpc_mpc_destroy(tpc_mpc_handle h);

/* Text of the last error on this handle (or of the last failed create when h == NULL). */
const char* tpc_mpc_last_error(tpc_mpc_handle h);

/* dlib::mpc<2,I,H> is a template: any horizon compiles.  Here every horizon 1 <= H <= 64 is accepted;
 * the ones this function lists (writes up to `cap`, returns how many exist) have kernels specialised
 * at compile time (LANE and WAVE), every other one runs a generic kernel with H as a
 * run-time value -- the same arithmetic, the same results (fp64: bit for bit), several times slower. */
int tpc_mpc_supported_horizons(int* out, int cap);
int tpc_mpc_abi_version(void);
/* How this binary was made: ABI version, target, and the LLVM machine scheduler each per-horizon
 * kernel unit was compiled with (csrc/Makefile).  Static text, valid for the process lifetime. */
const char* tpc_mpc_build_info(void);

/* ---- the call being replaced ------------------------------------------------------------------ */

/* Replaces the body of
 *   void TrajectoryPointController::mpcControllerTobi(double v, double delta_y, double delta_phi,
 *                                                      double* steering_front, double* steering_rear)
 * (include/trajectory_point_follower.h:44, src/trajectory_point_follower.cpp:301-389): builds
 * A=[1,Tv;0,1], B=[0,Tv;Tv/l,-Tv/l], C=0, Q, R from `p`, a fresh controller, one target
 * (delta_y, delta_phi) for all steps, x0 = 0, cold start, and returns u0.  `v` is the speed AFTER
 * the module's velocity lookup (src/...follower.cpp:323).  One instance on the GPU (WAVE kernel),
 * served by a resident wavefront that takes requests through a mailbox (see tpc_mpc_set_resident),
 * so the call costs no kernel launch and no synchronisation call -- or, on a host-only handle (TPC_MPC_DEVICE_NONE)
 * and for the horizons TPC_MPC_OPT_HOST_SOLVE_ONE names, on the calling thread (csrc/tpc_mpc_host.cpp). */
int tpc_mpc_solve_one(tpc_mpc_handle h, const tpc_mpc_params* p, double v, double delta_y,
                      double delta_phi, double* steering_front, double* steering_rear);

/* What the last tpc_mpc_solve_one on this handle reported beside its two outputs: the non-fatal flags the
 * batch entries return through flags_out (TPC_MPC_FLAG_NONFINITE: a NaN / Inf speed or target, the call returned
 * dlib's untouched start point (0, 0); TPC_MPC_FLAG_MAX_ITER: the solve was cut off by max_iter) and the
 * iteration count.  The reference's counterpart is the NaN check and log line behind the call
 * (src/trajectory_point_follower.cpp:101-103); dlib itself reports nothing (mpc.h:298-311).  Either pointer
 * may be NULL.  Costs nothing: the resident wavefront stores the word with its outputs.  TPC_MPC_ERR_BAD_ARG
 * before the first solve_one. */
int tpc_mpc_last_flags(tpc_mpc_handle h, uint32_t* flags, int32_t* iters);

/* No reference counterpart.  tpc_mpc_solve_one keeps one wavefront resident on the GPU between
 * calls (fp64, the specialised horizons, algo AUTO or WAVE; other requests take an ordinary launch).
 * The wavefront leaves by itself `idle_timeout_us` after its last request (default 20 000) and is
 * started again by the next call; tpc_mpc_destroy stops it.  While it is resident a device-wide
 * synchronisation elsewhere in the process (hipDeviceSynchronize, hipFree) waits for it, i.e. up to
 * the idle timeout.  idle_timeout_us <= 0 turns the resident mode off: every solve_one is then one
 * kernel launch.
 * Where the CPU can write device memory (hipDeviceAttributeIsLargeBar) the request is written into
 * device memory through the BAR, otherwise into pinned host memory (TPC_MPC_OPT_MAILBOX_HOST forces the
 * latter). */
int tpc_mpc_set_resident(tpc_mpc_handle h, int64_t idle_timeout_us);

/* The same computation for n independent instances in one launch.  Arrays are `p->dtype`,
 * length n, in `mem`.  `iters` (int32, optional) receives each instance's iteration count,
 * `flags_out` (optional) the OR of the per-instance flags.  `stream` is a hipStream_t or NULL;
 * with TPC_MPC_DEVICE memory the call is asynchronous on that stream unless flags_out != NULL
 * (reading the flags synchronises). */
int tpc_mpc_solve_batch_compact(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n,
                                const void* v, const void* delta_y, const void* delta_phi,
                                void* steering_front, void* steering_rear, int32_t* iters,
                                uint32_t* flags_out, int mem, void* stream);

/* Mixed-horizon batch (BASELINE.json config 5): instance k is solved with horizon horizons[k]
 * (int32, in `mem` like the other arrays); p->horizon is ignored.  The batch is binned by horizon on
 * the device, every bin runs its horizon's kernels, and the outputs come back in the caller's
 * order.  Only the specialised horizons (tpc_mpc_supported_horizons()) can be mixed: any other value
 * anywhere in the batch fails the call with TPC_MPC_ERR_BAD_HORIZON before anything is solved.  Unlike tpc_mpc_solve_batch_compact this call
 * synchronises `stream` once internally (the bin sizes decide the launches). */
int tpc_mpc_solve_batch_compact_mixed(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n,
                                      const int32_t* horizons, const void* v, const void* delta_y,
                                      const void* delta_phi, void* steering_front, void* steering_rear,
                                      int32_t* iters, uint32_t* flags_out, int mem, void* stream);

/* ---- the general dlib::mpc<2,I,H> surface ------------------------------------------------------- */

/* Per-instance model and state, SoA with leading dimension ld (see header comment):
 *   A[4]  row-major 2x2          B[2*I] row-major 2xI       C[2]  Q[2]  R[I]  lower[I]  upper[I]
 *   x0[2] current_state          targets[H*2]  (step t, state s at component 2*t+s;
 *                                               dlib::mpc::set_target(val,time), mpc.h:142-155)
 *   controls_inout[H*I] optional: the controller's stored controls (mpc.h:363).  As in
 *        operator() (mpc.h:229-239) they are shifted left by one step before the solve (warm
 *        start); on return they hold the solved sequence.  NULL = fresh controller (zeros).
 *   v_inout[H*I] optional: dlib's accelerated-gradient memory (mpc.h:250), which persists across
 *        calls of one controller object.  NULL = zeros in, not written.
 *   u0[I] out: controls[0], what operator() returns.
 * The caller shifts `targets` between calls (mpc.h:236-237) -- tpc_mpc_rollout does it on device. */
typedef struct tpc_mpc_general_io {
    int32_t inputs;           /* I: 1 or 2 */
    int32_t reserved;
    int64_t n, ld;
    const void *A, *B, *C, *Q, *R, *lower, *upper, *x0, *targets;
    void *controls_inout, *v_inout;
    void* u0;
    int32_t* iters;           /* optional */
} tpc_mpc_general_io;

/* Replaces: dlib::mpc<2,I,H> ctor (mpc.h:51-125) + set_target (mpc.h:142-155) + operator()
 * (mpc.h:216-240) for n independent controllers.  Uses p->horizon, dtype, algo, eps, max_iter,
 * smo_iters; the compact-model fields of `p` are ignored. */
int tpc_mpc_solve_batch_general(tpc_mpc_handle h, const tpc_mpc_params* p,
                                const tpc_mpc_general_io* io, uint32_t* flags_out, int mem,
                                void* stream);

/* Inputs and outputs of tpc_mpc_solve_batch_general_backward, SoA with the io's leading dimension ld:
 *   controls[H*I]       the solved sequence, as tpc_mpc_solve_batch_general returns it in controls_inout
 *   grad_controls[H*I]  dL/du: the gradient of the caller's loss with respect to those controls
 *   dA[4] dB[2*I] dC[2] dQ[2] dR[I] dlower[I] dupper[I] dx0[2] dtargets[H*2]
 *                       optional outputs, dL/d(the io array of the same name and shape); overwritten; NULL = not computed
 *   kkt_residual[1]     optional output: max |df| over the free components at `controls` (0 when none is free) */
typedef struct tpc_mpc_general_grad {
    const void *controls, *grad_controls;
    void *dA, *dB, *dC, *dQ, *dR, *dlower, *dupper, *dx0, *dtargets;
    void* kkt_residual;
} tpc_mpc_general_grad;

/* No reference counterpart (dlib::mpc has no derivative).  The backward pass of tpc_mpc_solve_batch_general: for n
 * instances, the gradient of a loss L(u) with respect to every model input, given the controls u and dL/du.
 *   Definition.  Component (t, j) of u is ACTIVE iff u[t,j] <= lower[j] or u[t,j] >= upper[j] (the comparisons of
 *   mpc.h:298-299 without the sign of the gradient; lower == upper is always active); the others form F.  The map
 *   differentiated holds the active components on their bounds and the free ones at the stationary point of dlib's QP
 *   on F: u_F = -H_FF^-1 (MM_F + H_FA u_A), with H and MM as in mpc.h:255-283.  If u is the exact optimum this is the
 *   derivative of the optimum; dlib's default eps (0.01) leaves a loose u, for which it is the derivative of the optimum
 *   on u's active set -- a small eps gives accurate gradients, and kkt_residual says how close u is.
 *   Method.  The adjoint direction w = H_FF^-1 dL/du_F (w = 0 on the active set) comes from a masked Riccati (LQR)
 *   sweep over the horizon, not from a dense Hessian: O(H) per instance, one lane each (csrc/mpc_grad_model.h).
 *   The per-step factors live in device scratch of the handle.
 * io: as for tpc_mpc_solve_batch_general; its controls_inout, v_inout, u0 and iters are ignored.  p is checked as for
 * the solve; what the backward pass uses of it is the horizon (1..64) and the dtype, which must be TPC_MPC_F64
 * (TPC_MPC_ERR_BAD_ARG otherwise).  Supported: every horizon 1..64, one or two inputs.
 * An instance with NaN / Inf inputs, controls or grad_controls (bounds may be infinite) raises TPC_MPC_FLAG_NONFINITE,
 * one that breaks dlib's requires clause TPC_MPC_FLAG_BAD_MODEL; such an instance gets all-zero gradients and a zero
 * residual.  Memory, stream and flags as tpc_mpc_solve_batch_general (HOST arrays are staged; with DEVICE memory the
 * call is asynchronous on `stream` unless flags_out != NULL).  A host-only handle (TPC_MPC_DEVICE_NONE) runs HOST
 * batches on the calling thread, in the same arithmetic bit for bit, and returns TPC_MPC_ERR_NO_DEVICE for DEVICE. */
int tpc_mpc_solve_batch_general_backward(tpc_mpc_handle h, const tpc_mpc_params* p,
                                         const tpc_mpc_general_io* io, const tpc_mpc_general_grad* g,
                                         uint32_t* flags_out, int mem, void* stream);

/* Parameters and per-instance outputs of tpc_mpc_polish_batch_general:
 *   tol           the residual a polished sequence must reach: dlib's eps (the same quantity, see below); > 0
 *   max_rounds    Newton rounds allowed per instance; >= 0 (0 only verifies)
 *   status        optional, int32 [n]: the rounds the instance used (0 = it already passed), or -1 = not polished
 *   residual_in   optional, fp64 [n]: res of the clamped input sequence
 *   residual_out  optional, fp64 [n]: res of the returned sequence (= residual_in for status -1) */
typedef struct tpc_mpc_polish {
    double tol;
    int32_t max_rounds;
    int32_t reserved;
    int32_t* status;
    void *residual_in, *residual_out;
} tpc_mpc_polish;

/* No reference counterpart.  Polish: moves a control sequence of dlib's box QP -- typically what
 * tpc_mpc_solve_batch_general left in controls_inout at dlib's default eps -- onto the exact minimiser whenever that
 * can be reached and VERIFIED in a few Newton rounds, and leaves it as it was otherwise.
 *   Definition.  With dlib's df = H u + MM (mpc.h:255-283) and its mask (mpc.h:298-299): component (t, j) is BLOCKED
 *   iff (u <= lower_j && df > 0) || (u >= upper_j && df < 0), or lower_j == upper_j; F is the rest.
 *   res(u) = max |df| over F (0 when F is empty) -- the quantity dlib's stop test compares with eps.
 *     u <- clamp(u, lower, upper)
 *     for round = 0 .. max_rounds:
 *         df, F, res from u
 *         if res <= tol: status = round; return u
 *         if round == max_rounds: break
 *         safeguard: if the previous round was a regular one and res did not fall below its res, this round is an
 *                    INNER round: the components on a bound leave F (they stay on the bound); the round after an
 *                    inner round is regular again
 *         w = H_FF^-1 df_F  (w = 0 off F);  u_F <- clamp(u_F - w_F, lower, upper)
 *     status = -1; the caller's sequence is returned bit for bit
 *   H is positive definite (R > 0), so a u with res(u) <= tol under this mask is a KKT point of the convex QP to that
 *   tolerance: the acceptance test is the proof, whatever path led there.
 *   Method.  df by dlib's two recurrences, w by the masked Riccati sweep of the backward pass
 *   (csrc/mpc_polish_model.h on csrc/mpc_grad_model.h): O(H) per round, one lane per instance, every round in one launch.
 * io: as for tpc_mpc_solve_batch_general.  controls_inout is required: in = the sequence to polish (NOT shifted), out =
 * the result; u0 (optional here) receives row 0 of the result; v_inout and iters are ignored.  p: as for the solve;
 * used are the horizon (1..64) and the dtype, which must be TPC_MPC_F64 (TPC_MPC_ERR_BAD_ARG otherwise); one or two
 * inputs.  q->tol <= 0 (or NaN) or q->max_rounds < 0: TPC_MPC_ERR_BAD_ARG.
 * An instance with NaN / Inf data or sequence (TPC_MPC_FLAG_NONFINITE; bounds may be infinite) or a model that breaks
 * dlib's requires clause (TPC_MPC_FLAG_BAD_MODEL) is not touched: status -1, residuals 0.  Any other instance that
 * returns -1 raises TPC_MPC_FLAG_NOT_POLISHED.  Memory, stream, flags and the host-only handle as
 * tpc_mpc_solve_batch_general_backward (HOST arrays are staged; a host-only handle runs HOST batches on the calling
 * thread with the kernel's bits). */
#define TPC_MPC_FLAG_NOT_POLISHED 0x8u
int tpc_mpc_polish_batch_general(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                 const tpc_mpc_polish* q, uint32_t* flags_out, int mem, void* stream);

/* Closed loop on device: `steps` successive operator() calls per controller with warm start and
 * target shift (mpc.h:229-239), plant update x <- A x + B u + C between calls (the loop of
 * dlib_files/dlib/test/mpc.cpp:301-316).  io->x0 is the initial state and is left untouched;
 * io->targets holds the initial H targets; new_last_targets (optional, SoA [steps*2] per
 * instance) supplies set_last_target() values for steps >= 1 (NULL repeats the last target).
 * controls_out: SoA [steps*I]; states_out (optional): SoA [steps*2]; iters_out (optional, int32):
 * SoA [steps].  io->controls_inout / v_inout (optional) carry the controller state in and out. */
int tpc_mpc_rollout(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                    int32_t steps, const void* new_last_targets, void* controls_out,
                    void* states_out, int32_t* iters_out, uint32_t* flags_out, int mem,
                    void* stream);

/* tpc_mpc_rollout that also records every step's solved sequence, for tpc_mpc_rollout_backward.
 * sequences_out (required): SoA [steps*H*I]; step k's sequence U_k (what controls_inout holds after the k-th
 * operator() call, mpc.h:229-239) is rows k*H*I .. (k+1)*H*I-1 in the controls_inout order.  Everything else, the bits
 * of every output included, is tpc_mpc_rollout's (one implementation; tpc_mpc_rollout records nothing). */
int tpc_mpc_rollout_record(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                           int32_t steps, const void* new_last_targets, void* controls_out,
                           void* states_out, int32_t* iters_out, void* sequences_out, uint32_t* flags_out,
                           int mem, void* stream);

/* No reference counterpart.  The closed loop of tpc_mpc_rollout with the polish of tpc_mpc_polish_batch_general between
 * every solve and the plant update, so that every step returns the verified minimiser of its box QP (unique: R > 0)
 * and the loop is a function of its inputs that does not depend on eps, the warm start or the kernel family beyond tol.
 *   Definition.  Step k, per instance:
 *     U_k <- the solve of tpc_mpc_rollout's step k (shift of the controls, warm start, p's eps / max_iter / algo)
 *     U_k <- polish(U_k) with x_k, the shifted targets T_k, q->tol, q->max_rounds: the rule of
 *            tpc_mpc_polish_batch_general, unchanged -- an instance whose residual passes tol is written, any other
 *            keeps the solver's sequence
 *     u0_k = row 0 of U_k;  x_{k+1} = A x_k + B u0_k + C  (tpc_mpc_rollout's plant arithmetic, operation for operation)
 *     record u0_k, x_{k+1}, U_k, iters, status;  target shift and set_last_target as tpc_mpc_rollout
 *   The result equals, bit for bit, the loop a caller could write from tpc_mpc_solve_batch_general (controls_inout and
 *   v_inout carried), tpc_mpc_polish_batch_general and the plant update.
 *   v (dlib's accelerated-gradient memory, v_inout) is left as the solve wrote it: the polish moves the sequence only.
 *   The next solve reads v again only after dlib has reset it to the sequence at iteration 49 (mpc.h:328-334) -- except
 *   when dlib's Q_diag == 0 `continue` (mpc.h:322) skips that reset at iteration 49: the projected-gradient steps then
 *   start from the v of the previous call, which belongs to the unpolished sequence.  The polished loop is still the
 *   composition above, since the composition carries the same v.
 *   Method.  Per step the solve dispatch, then ONE kernel (csrc/mpc_rollout_polish.hip), one lane per instance: every
 *   polish round in the lane, then the step tail of tpc_mpc_rollout without leaving it.
 * q: tol > 0 and max_rounds >= 0 as in tpc_mpc_polish_batch_general (TPC_MPC_ERR_BAD_ARG otherwise, also for a null q).
 *   q->status (int32), q->residual_in, q->residual_out (fp64) are optional and hold one row per step here: SoA [steps]
 *   with the io's ld, like iters_out.  An (instance, step) pair the polish cannot verify keeps the solver's sequence for
 *   that step, gets status -1 in that step's row and raises TPC_MPC_FLAG_NOT_POLISHED; the loop goes on from it.  An
 *   instance with non-finite data or a model that breaks dlib's requires clause behaves as in tpc_mpc_rollout (its
 *   rows, TPC_MPC_FLAG_NONFINITE / _BAD_MODEL), gets status -1 and residuals 0 in every step and does not raise
 *   TPC_MPC_FLAG_NOT_POLISHED by itself.
 * sequences_out is optional (NULL: not recorded); when given it holds the polished sequences in
 * tpc_mpc_rollout_record's layout, i.e. exactly what tpc_mpc_rollout_backward is to be given together with states_out.
 * io->controls_inout / v_inout (optional) carry the controller state in and out as in tpc_mpc_rollout (controls out =
 * the last step's polished sequence).  Everything else as tpc_mpc_rollout.  fp64 only (p->dtype other than TPC_MPC_F64:
 * TPC_MPC_ERR_BAD_ARG), horizons 1..64, one or two inputs.  n == 0 or steps == 0 returns TPC_MPC_OK with flags 0.
 * Like the other closed loops it needs the device: a host-only handle (TPC_MPC_DEVICE_NONE) returns
 * TPC_MPC_ERR_NO_DEVICE, after the argument checks above. */
int tpc_mpc_rollout_polished(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                             int32_t steps, const void* new_last_targets, const tpc_mpc_polish* q,
                             void* controls_out, void* states_out, int32_t* iters_out, void* sequences_out,
                             uint32_t* flags_out, int mem, void* stream);

/* No reference counterpart.  The polished closed loop with the Newton rounds FIRST: the polish is an active-set Newton
 * method that carries its own proof (a sequence whose residual passes tol under dlib's mask is the unique minimiser,
 * whatever produced it), so the first-order solve is needed only where the polish does not verify from the shifted
 * warm start.  An instance the polish verifies at every step costs no solve at all, and the whole loop of such
 * instances is ONE kernel launch (csrc/mpc_rollout_newton.hip, one lane per instance, all steps).
 *   Phase 1, the Newton pass.  Per instance, for k = 0 .. steps-1:
 *     U   <- dlib's shift of the carried controls (mpc.h:231-232), at step 0 too, exactly as tpc_mpc_rollout does it;
 *            the start is io->controls_inout, zeros when that is NULL
 *     U   <- polish(U) at x_k with the shifted targets T_k, q->tol, q->max_rounds: the rule of
 *            tpc_mpc_polish_batch_general, unchanged
 *     not verified (the polish's status -1): the instance stops here, first_unverified = k, and this phase writes none
 *            of its rows of step k and later
 *     verified: u0_k = row 0 of U;  x_{k+1} = A x_k + B u0_k + C in tpc_mpc_rollout's plant arithmetic;  record u0_k,
 *            x_{k+1}, U_k, status = the rounds used, the residual rows, iters_out 0;  target shift and set_last_target
 *            as tpc_mpc_rollout
 *   An instance verified at every step gets first_unverified = steps.  A verified step equals, bit for bit,
 *   tpc_mpc_polish_batch_general on the shifted sequence followed by tpc_mpc_rollout's step.
 *   Phase 2, fallback TPC_MPC_NEWTON_FALLBACK_SOLVE.  The instances with first_unverified < steps are gathered into a
 *   compact batch, run from step 0 through tpc_mpc_rollout_polished's loop (p's eps / max_iter / algo, the same q), and
 *   every output row of theirs -- v included -- is scattered back: their outputs are exactly what
 *   tpc_mpc_rollout_polished returns for the gathered batch.  They raise TPC_MPC_FLAG_NOT_POLISHED only for
 *   (instance, step) pairs that loop itself leaves at -1.  first_unverified keeps phase 1's value, so the caller sees
 *   who fell back.  The order of the instances inside the compact batch is not defined.  One 4-byte read-back (the
 *   number of such instances) sits between the phases; there is no other host synchronisation inside the loop.
 *   Fallback TPC_MPC_NEWTON_FALLBACK_NONE.  Phase 1 only: the rows of an unverified instance from first_unverified on
 *   get status -1, residuals 0 and zero controls / states / sequences / iters, the instance raises
 *   TPC_MPC_FLAG_NOT_POLISHED, and its controls_inout / v_inout come back zero (the last step's sequence row).
 *   Controller state out.  controls_inout is the last step's sequence.  v_inout of an instance phase 1 carried through
 *   is set equal to that sequence -- the value dlib itself resets v to (mpc.h:328-334); a fallback instance's v is
 *   whatever the polished loop left.
 *   Invalid instances (non-finite data, or a model that breaks dlib's requires clause; also a state that stops being
 *   finite at a later step) keep their TPC_MPC_FLAG_NONFINITE / _BAD_MODEL, stop at that step like an unverified one
 *   (first_unverified = the step, rows as under FALLBACK_NONE), are NOT sent to the fallback under either mode and do
 *   not raise TPC_MPC_FLAG_NOT_POLISHED by themselves.
 * Arguments as tpc_mpc_rollout_polished, plus `fallback` and the optional first_unverified (int32 [n], NULL: not
 * returned).  q->status / residual_in / residual_out hold one row per step.  A null q, tol <= 0, max_rounds < 0, an
 * unknown fallback or a dtype other than TPC_MPC_F64 return TPC_MPC_ERR_BAD_ARG.  fp64 only, horizons 1..64, one or
 * two inputs.  n == 0 or steps == 0 returns TPC_MPC_OK with flags 0.
 * A host-only handle (TPC_MPC_DEVICE_NONE) runs FALLBACK_NONE on the calling thread with the kernel's bits (HOST memory
 * only), as tpc_mpc_polish_batch_general does; with FALLBACK_SOLVE it returns TPC_MPC_ERR_NO_DEVICE, after the argument
 * checks above. */
#define TPC_MPC_NEWTON_FALLBACK_SOLVE 0
#define TPC_MPC_NEWTON_FALLBACK_NONE 1
int tpc_mpc_rollout_newton(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                           int32_t steps, const void* new_last_targets, const tpc_mpc_polish* q, int32_t fallback,
                           void* controls_out, void* states_out, int32_t* iters_out, void* sequences_out,
                           int32_t* first_unverified, uint32_t* flags_out, int mem, void* stream);

/* No reference counterpart.  mpcControllerTobi for n instances with the VERIFIED OPTIMUM as the answer, not dlib's
 * eps-0.01 point: the polish's Newton rounds from a cold start, the first-order solve only where they do not verify.
 * Instance k has the general-form model the reference controller builds from (v, delta_y, delta_phi)
 * (src/trajectory_point_follower.cpp:326-371), with T = p->step_size, l = p->wheelbase, Tv = T * v:
 *     A = [1, Tv; 0, 1]   B = [0, Tv; Tv/l, -Tv/l] (Tv/l: one multiply, one divide)   C = 0   x0 = 0
 *     Q = (weight_y, weight_phi)   R = (weight_steering_front, weight_steering_rear)   lower, upper from p
 *     every one of the H targets (delta_y, delta_phi)
 *   Phase 1, every instance.  U <- polish(U = 0) by the rule of tpc_mpc_polish_batch_general, unchanged, with q->tol and
 *   q->max_rounds, in ONE launch that reads three doubles and writes two per instance (csrc/mpc_newton_compact.hip; at
 *   horizons 4 and 5 the per-step values stay in registers and no workspace memory is touched).
 *     verified: steering_front / steering_rear = row 0 of U, sequence_out = U, status = the rounds used, and the two
 *            residuals.  All of them equal, bit for bit (signed zeros included), what tpc_mpc_polish_batch_general
 *            returns for the expanded arrays with zero controls.
 *   Phase 2, fallback TPC_MPC_NEWTON_FALLBACK_SOLVE.  The unverified instances are gathered and expanded to the general
 *   form on the device (those instances only), solved cold with p's eps / max_iter / smo_iters / algo as
 *   tpc_mpc_solve_batch_general does with zeroed controls_inout, polished with the same q and scattered back: their
 *   outputs are exactly what those two entries return for the gathered batch.  status -1 and
 *   TPC_MPC_FLAG_NOT_POLISHED are raised only where that polish also fails; the solver's u0 and sequence are then
 *   returned.  fell_back[k] = 1 for them, 0 for everyone else.  The order of the instances inside the gathered batch is
 *   not defined.  One 4-byte read-back (the number of such instances) sits between the phases.
 *   Fallback TPC_MPC_NEWTON_FALLBACK_NONE.  Phase 1 only: an unverified instance returns (0, 0), a zero sequence,
 *   status -1, residual_out 0 (residual_in: the residual at U = 0) and raises TPC_MPC_FLAG_NOT_POLISHED.  With
 *   flags_out == NULL and DEVICE memory the call is asynchronous.
 *   Invalid instances.  A non-finite v, delta_y or delta_phi (or a model value that stops being finite) raises
 *   TPC_MPC_FLAG_NONFINITE; the instance returns (0, 0), a zero sequence, status -1 and zero residuals, is NOT sent to
 *   the fallback and does not raise TPC_MPC_FLAG_NOT_POLISHED by itself.
 * p is validated as tpc_mpc_solve_batch_compact validates it.  q->status (int32), q->residual_in, q->residual_out and
 * fell_back (int32) are optional rows [n]; sequence_out is optional, SoA [H*2] with leading dimension n.  A null q,
 * tol <= 0 (or NaN), max_rounds < 0, an unknown fallback or a dtype other than TPC_MPC_F64 return TPC_MPC_ERR_BAD_ARG.
 * fp64 only, horizons 1..64.  n == 0 returns TPC_MPC_OK with flags 0.  HOST arrays are staged: three rows in, two
 * (+ 2H and the optional rows) out.
 * A host-only handle (TPC_MPC_DEVICE_NONE) runs FALLBACK_NONE on the calling thread with the kernel's bits (HOST memory
 * only); with FALLBACK_SOLVE it returns TPC_MPC_ERR_NO_DEVICE, after the argument checks above. */
int tpc_mpc_solve_batch_compact_exact(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                      const void* delta_y, const void* delta_phi, const tpc_mpc_polish* q,
                                      int32_t fallback, void* steering_front, void* steering_rear, void* sequence_out,
                                      int32_t* fell_back, uint32_t* flags_out, int mem, void* stream);

/* The incoming gradient and the outputs of tpc_mpc_solve_batch_compact_exact_backward, fp64.  The ten shared
 * parameters are indexed 0 weight_y, 1 weight_phi, 2 weight_steering_front, 3 weight_steering_rear, 4 step_size,
 * 5 wheelbase, 6 lower[0], 7 lower[1], 8 upper[0], 9 upper[1]. */
typedef struct tpc_mpc_compact_grad {
    const void *grad_front, *grad_rear;   /* [n] dL/dsteering_front, dL/dsteering_rear; either may be NULL (zero) */
    const void *grad_sequence;            /* optional [H*2], ld n: dL/dsequence_out; NULL (zero)                  */
    void *dv, *ddelta_y, *ddelta_phi;     /* optional outputs [n]                                                 */
    void *dparams_rows;                   /* optional output [10], ld n: per-instance dL/d(shared parameter)      */
    void *dparams;                        /* optional output [10]: their sum over the batch                       */
    void *kkt_residual;                   /* optional output [n], as tpc_mpc_general_grad                         */
} tpc_mpc_compact_grad;

/* No reference counterpart.  The backward pass of tpc_mpc_solve_batch_compact_exact: for n instances that share p's
 * weights, step_size, wheelbase and bounds, the gradient of a loss L(steering_front, steering_rear, sequence_out) with
 * respect to v, delta_y, delta_phi and those ten shared parameters, without the general form ever being written.
 *   Definition.  Instance k has the expanded model of tpc_mpc_solve_batch_compact_exact (T = p->step_size,
 *   l = p->wheelbase, Tv = T * v: A = [1, Tv; 0, 1], B = [0, Tv; Tv/l, -Tv/l], C = 0, x0 = 0, every target
 *   (delta_y, delta_phi)).  Its incoming gradient is g(t, j) = grad_sequence[t*2+j], plus grad_front at (0, 0) and
 *   grad_rear at (0, 1), added in the order grad_sequence + grad_front; an absent array counts as +0.0.  The adjoint
 *   sweep of tpc_mpc_solve_batch_general_backward (csrc/mpc_grad_model.h, qp_step<2>, unchanged) runs on that model,
 *   `sequence` and g; call its sums s (dA, dB, dQ, dR, dlower, dupper, kkt of that entry) and its dL/dtarget_t
 *   (a_t, b_t), which arrive with t from H-1 down to 0.  Then, every operation rounded on its own:
 *     S = s.A01 + s.B0[1]      D = s.B1[0] - s.B1[1]      Tv = T * v
 *     dv         = T * S + (T / l) * D
 *     ddelta_y   = ((0.0 + a_{H-1}) + a_{H-2}) + ... + a_0          ddelta_phi likewise with b_t
 *     rows[0..3] = s.Q0, s.Q1, s.R[0], s.R[1]
 *     rows[4]    = v * S + (v / l) * D                               (step_size)
 *     rows[5]    = -((Tv / l) / l) * D                               (wheelbase)
 *     rows[6..9] = s.lo[0], s.lo[1], s.hi[0], s.hi[1]
 *     kkt_residual = s.kkt
 *   These equal, bit for bit up to the sign of a zero, tpc_mpc_solve_batch_general_backward on the expanded arrays pushed
 *   through the same lines.  dparams[c] is the sum of rows[c] over the contributing instances.
 *   Excluded instances.  status != NULL && status[k] < 0 (nobody should differentiate the (0, 0) that stands in for an
 *   unverified instance); a non-finite v, target, sequence, g or model value (TPC_MPC_FLAG_NONFINITE); a model that
 *   breaks dlib's requires clause (TPC_MPC_FLAG_BAD_MODEL).  An excluded instance gets 0.0 in every per-instance output
 *   and adds nothing to dparams; a negative status raises no flag of its own.
 *   Method.  One lane per instance (csrc/mpc_compact_grad.hip): 3 + 2H doubles and the incoming gradient in, three
 *   doubles out; the per-step values in the handle's gradient workspace, at horizons 4 and 5 in registers.  dparams
 *   is summed without floating-point atomics: a fixed butterfly inside a wavefront, the block's wavefronts in order,
 *   one partial row per block, one single-block launch over the blocks in a fixed order -- the same call on the same
 *   data returns the same bytes every time.  The order depends on n; it is not the ascending-k order.
 * p is validated as tpc_mpc_solve_batch_compact validates it.  v, delta_y, delta_phi [n] and sequence (SoA [H*2], leading
 * dimension n, as sequence_out) are required; status (int32 [n]) is optional.  fp64 only, horizons 1..64.  A null g, a
 * null sequence or a dtype other than TPC_MPC_F64 return TPC_MPC_ERR_BAD_ARG.  n == 0 returns TPC_MPC_OK with flags 0
 * and writes zeros to dparams.  HOST arrays are staged; with DEVICE memory and flags_out == NULL the call is
 * asynchronous on `stream`.  A host-only handle (TPC_MPC_DEVICE_NONE) runs HOST batches on the calling thread with the
 * kernel's per-instance bits, its dparams summed in ascending k, and returns TPC_MPC_ERR_NO_DEVICE for DEVICE memory. */
int tpc_mpc_solve_batch_compact_exact_backward(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                               const void* delta_y, const void* delta_phi,
                                               const void* sequence /* [H*2], ld n */,
                                               const int32_t* status /* optional [n] */,
                                               const tpc_mpc_compact_grad* g, uint32_t* flags_out, int mem,
                                               void* stream);

/* No reference counterpart.  tpc_mpc_solve_batch_compact_exact and its backward pass with PER-INSTANCE weights,
 * step_size, wheelbase and bounds: weights scheduled on speed, logs recorded with different wheelbases or cycle times,
 * per-instance steering limits -- still without the general form being written for the instances that verify.
 *   params_rows.  Required (NULL: TPC_MPC_ERR_BAD_ARG), SoA fp64 [10] with leading dimension n, in `mem` like every
 *   other array: element (c, k) at base[c*n + k] is parameter c of instance k, c in the order of tpc_mpc_compact_grad
 *   (0 weight_y, 1 weight_phi, 2 weight_steering_front, 3 weight_steering_rear, 4 step_size, 5 wheelbase, 6 lower[0],
 *   7 lower[1], 8 upper[0], 9 upper[1]).  HOST rows are staged with v.
 *   p gives the horizon, dtype, eps / max_iter / smo_iters / algo / options only; its ten model fields are neither read
 *   nor validated.
 *   Forward.  Instance k has the model of tpc_mpc_solve_batch_compact_exact built from v[k] and column k, by the same
 *   rounded operations (Tv = T_k * v_k, Tv / l_k, its negation).  Phase 1 equals, bit for bit, what
 *   tpc_mpc_polish_batch_general returns for the per-instance expanded arrays with zero controls; phase 2 gathers and
 *   expands the unverified instances with their own ten values, and is what tpc_mpc_solve_batch_general and
 *   tpc_mpc_polish_batch_general return for exactly those.  With every row constant along n, every output equals, bit
 *   for bit, tpc_mpc_solve_batch_compact_exact called with those ten values in p.
 *   Invalid instances are decided per instance.  TPC_MPC_FLAG_NONFINITE: a non-finite v, target, weight, step_size or
 *   wheelbase, a NaN bound, a non-finite Tv or Tv / l (wheelbase == 0 lands here).  TPC_MPC_FLAG_BAD_MODEL: a negative
 *   weight_y / weight_phi, a steering weight <= 0, upper < lower (a NaN weight or bound fails these comparisons too and
 *   raises both flags, as it does in the general form).  Infinite bounds are legal.  Forward: (0, 0), a zero
 *   sequence, status -1, zero residuals, not sent to the fallback, no TPC_MPC_FLAG_NOT_POLISHED of its own.  Backward:
 *   excluded -- zeros in every per-instance output, nothing added to dparams.
 *   Backward.  The definition of tpc_mpc_solve_batch_compact_exact_backward, line for line, with T, l and the model
 *   from column k.  dparams_rows [10], ld n, is the gradient with respect to instance k's OWN ten parameters; dparams
 *   [10] stays their column sum over the contributing instances, by the same fixed-order reduction -- the gradient of
 *   a parameter the caller broadcast to every instance.  With constant rows every output equals the shared entry's bits.
 * Everything else -- the argument checks, n == 0, the optional outputs, asynchronous DEVICE calls with flags_out == NULL,
 * the host-only handle -- is as the two entries above have it.  Kernels: the ROWS instantiations of the parents'
 * (csrc/mpc_newton_compact.hip, csrc/mpc_compact_grad.hip), one lane per instance, the ten values loaded once per lane. */
int tpc_mpc_solve_batch_compact_exact_rows(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                           const void* delta_y, const void* delta_phi,
                                           const void* params_rows /* [10], ld n */, const tpc_mpc_polish* q,
                                           int32_t fallback, void* steering_front, void* steering_rear,
                                           void* sequence_out, int32_t* fell_back, uint32_t* flags_out, int mem,
                                           void* stream);
int tpc_mpc_solve_batch_compact_exact_rows_backward(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n,
                                                    const void* v, const void* delta_y, const void* delta_phi,
                                                    const void* params_rows /* [10], ld n */,
                                                    const void* sequence /* [H*2], ld n */,
                                                    const int32_t* status /* optional [n] */,
                                                    const tpc_mpc_compact_grad* g, uint32_t* flags_out, int mem,
                                                    void* stream);

/* No reference counterpart.  tpc_mpc_solve_batch_compact_exact / _exact_rows WARM-STARTED: the Newton rounds of phase 1
 * begin at a sequence the caller gives per instance -- in a fitting loop, the instance's own optimum from the previous
 * optimiser step (the sequence_out of that call) -- not at U = 0.  Near the optimum one round verifies where the cold
 * start needs two or three, and most of the instances the cold start sends to the fallback verify in phase 1.
 *   params_rows.  Optional, [10] with leading dimension n as tpc_mpc_solve_batch_compact_exact_rows takes it.  NULL: p's
 *   ten values, and every rule below is tpc_mpc_solve_batch_compact_exact's; given: the rows entry's (p's ten model
 *   fields neither read nor validated, invalid columns decided per instance).
 *   start.  Required (NULL: TPC_MPC_ERR_BAD_ARG), SoA fp64 [H*2] with leading dimension n, in `mem` like every other
 *   array: element (t*2+j, k) at base[(t*2+j)*n + k], the layout of sequence_out.  HOST rows are staged with v.
 *   Phase 1.  Instance k runs the parents' rounds with ONE change: the working copy begins at
 *   clamp(start[(t*2+j)*n + k], lower[j], upper[j]) where the parents begin at clamp(0.0, lower[j], upper[j]).  For an
 *   instance whose start is finite in every component, steering_front / steering_rear, sequence_out, status and both
 *   residuals equal, bit for bit, what tpc_mpc_polish_batch_general returns for the (per-instance) expanded arrays with
 *   controls = start; residual_in is the residual at the clamped start.
 *   No start.  An instance with a NaN or an Inf in ANY component of its start column is that instance of the cold
 *   entry, bit for bit: it starts from clamp(0.0, ..) in every component and raises no flag.  This is how a caller
 *   says "I have no start for this one"; a column of zeros gives the same result.
 *   Phase 2, the flags, invalid instances (their start is not read), the optional outputs, n == 0, the argument errors,
 *   asynchronous DEVICE calls with flags_out == NULL and the host-only handle are the parents'.  The fallback solves
 *   cold, as the parents' does: an instance that falls back returns what tpc_mpc_solve_batch_general and
 *   tpc_mpc_polish_batch_general return for it, whatever its start was.  Under TPC_MPC_NEWTON_FALLBACK_NONE an
 *   unverified instance returns (0, 0), a zero sequence and status -1, so the next call finds a column of zeros there.
 *   Aliasing.  sequence_out == start is allowed (update the stored sequences in place): a lane reads its whole column
 *   before its first write.  No other overlap of an input with an output is.
 * Kernels: the WARM instantiations of the parents' (csrc/mpc_newton_compact.hip), launched as the parents' -- one lane per instance, the
 * start loaded once; at horizons 4 and 5 the per-step values stay in registers. */
int tpc_mpc_solve_batch_compact_exact_from(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                           const void* delta_y, const void* delta_phi,
                                           const void* params_rows /* optional [10], ld n */,
                                           const void* start /* [H*2], ld n */, const tpc_mpc_polish* q,
                                           int32_t fallback, void* steering_front, void* steering_rear,
                                           void* sequence_out, int32_t* fell_back, uint32_t* flags_out, int mem,
                                           void* stream);

/* The K directions of tpc_mpc_solve_batch_compact_exact_forward, fp64: each a tangent of every input of
 * tpc_mpc_solve_batch_compact_exact.  A NULL array is a zero tangent.  The ten parameters are indexed as in
 * tpc_mpc_compact_grad. */
typedef struct tpc_mpc_compact_tangents {
    int32_t directions, reserved;           /* K >= 1, K * n < 2^31                                                  */
    const void *tv, *tdelta_y, *tdelta_phi; /* optional [K], ld n: element (d, k) at base[d*n + k]; NULL = zero      */
    const void *tparams;                    /* optional [K*10] ELEMENTS (not per instance), in `mem`, as dparams is
                                               [10]: element (d, c) at base[d*10 + c], the tangent of the ten shared
                                               parameters; without params_rows only                                   */
    const void *tparams_rows;               /* optional [K*10], ld n: (d, c, k) at base[(d*10 + c)*n + k]; needs
                                               params_rows                                                            */
} tpc_mpc_compact_tangents;

/* No reference counterpart.  The forward-mode derivative of tpc_mpc_solve_batch_compact_exact / _exact_rows: for K
 * directions, the tangents of steering_front, steering_rear and (optionally) sequence_out along a tangent of v,
 * delta_y, delta_phi and the ten parameters, without the general form ever being written.  It is what Gauss-Newton
 * and Levenberg-Marquardt fits of a few shared parameters to many residuals need: the per-instance Jacobian, K
 * columns per call.
 *   Definition.  Instance k, direction d.  T, l, q0, q1, r[2], lo[2], hi[2] come from p, or from column k of
 *   params_rows; the model is tpc_mpc_solve_batch_compact_exact's (Tv = T * v, tvl = Tv / l: A = [1, Tv; 0, 1],
 *   B = [0, Tv; tvl, -tvl], C = 0, x0 = 0, every target (delta_y, delta_phi)).  The direction's values are tv, tdy,
 *   tdphi and tp[0..9] = tq0, tq1, tr0, tr1, tT, tl, tlo0, tlo1, thi0, thi1; an absent array counts as +0.0.  Then,
 *   every operation rounded on its own:
 *     tTv  = tT * v + T * tv
 *     ttvl = (tTv - tvl * tl) / l
 *     tA = [0, tTv; 0, 0]      tB = [0, tTv; ttvl, -ttvl]      tC = 0      tx0 = 0
 *     tQ, tR, tlower, tupper = (tq0, tq1), (tr0, tr1), (tlo0, tlo1), (thi0, thi1);  every target's tangent (tdy, tdphi)
 *   and the tangent sweep of tpc_mpc_solve_batch_general_forward (csrc/mpc_tangent_model.h, step<2>, unchanged) runs
 *   on that model, that tangent and `sequence`: tsequence is its tU, tfront = tU(0, 0), trear = tU(0, 1).  These equal,
 *   as numbers (the sign of a zero is free), what tpc_mpc_solve_batch_general_forward returns for the expanded arrays
 *   and tangents.  When `sequence` is the optimum this is the derivative of the optimum; the map is the transpose of
 *   tpc_mpc_solve_batch_compact_exact_backward to rounding.
 *   Excluded.  status != NULL && status[k] < 0: every direction's block of instance k is zero, without a flag of its
 *   own.  A non-finite v, target, sequence or model value, or a non-finite tangent in direction d (given params_rows:
 *   a non-finite step_size or wheelbase too): TPC_MPC_FLAG_NONFINITE, and the (d, k) block is zero -- the other
 *   directions of k are not touched by one direction's tangent.  A model that breaks dlib's requires clause:
 *   TPC_MPC_FLAG_BAD_MODEL, and the (d, k) block is zero.
 *   params_rows == NULL: p's ten values, validated as tpc_mpc_solve_batch_compact_exact_backward validates them; a given
 *   t->tparams_rows is TPC_MPC_ERR_BAD_ARG.  params_rows given ([10], ld n): the rows entry's rules -- p's ten model
 *   fields neither read nor validated, invalid columns decided per instance; a given t->tparams is
 *   TPC_MPC_ERR_BAD_ARG.
 *   Method.  One lane per (direction, instance), L = d*n + k (csrc/mpc_compact_tangent.hip): 3 + 2H doubles and the
 *   direction's values in, two doubles out; the per-step values in the handle's gradient workspace, at horizons 4 and
 *   5 without tsequence in registers.  A tangent of shared parameters reads no per-instance tangent array.  The same
 *   bits with and without tsequence.
 * v, delta_y, delta_phi [n] and sequence (SoA [H*2], ld n, as sequence_out) are required; status (int32 [n]) is
 * optional.  Outputs: tfront, trear [K] with ld n (element (d, k) at base[d*n + k]) and tsequence [K*2H] with ld n
 * (element (d, t*2+j, k) at base[(d*2H + t*2+j)*n + k]); each may be NULL, not all three.  fp64 only, horizons 1..64.
 * TPC_MPC_ERR_BAD_ARG: a null t, a null sequence or batch pointer, directions < 1 or directions * n >= 2^31, all
 * three outputs NULL, a dtype other than TPC_MPC_F64.  n == 0 returns TPC_MPC_OK with flags 0.  HOST arrays are
 * staged; with DEVICE memory and flags_out == NULL the call is asynchronous on `stream`.  A host-only handle
 * (TPC_MPC_DEVICE_NONE) runs HOST batches on the calling thread with the kernel's bits and returns
 * TPC_MPC_ERR_NO_DEVICE for DEVICE memory.  No output may overlap an input. */
int tpc_mpc_solve_batch_compact_exact_forward(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                              const void* delta_y, const void* delta_phi,
                                              const void* params_rows /* optional [10], ld n */,
                                              const void* sequence /* [H*2], ld n */,
                                              const int32_t* status /* optional [n] */,
                                              const tpc_mpc_compact_tangents* t, void* tfront /* [K], ld n */,
                                              void* trear /* [K], ld n */, void* tsequence /* optional [K*2H], ld n */,
                                              uint32_t* flags_out, int mem, void* stream);

/* No reference counterpart.  The compact closed loop: mpcControllerTobi's controller rolled forward `steps` steps on its
 * own model, every step answered with the VERIFIED OPTIMUM -- tpc_mpc_rollout_newton on the model that
 * tpc_mpc_solve_batch_compact_exact builds, without the general form: three doubles (+ x0) in per instance, two (+ the
 * optional rows) out per step, the model built in registers.
 * Instance k has tpc_mpc_solve_batch_compact_exact's model, with T = p->step_size, l = p->wheelbase, Tv = T * v:
 *     A = [1, Tv; 0, 1]   B = [0, Tv; Tv/l, -Tv/l]   C = 0   Q, R, lower, upper from p
 *     every one of the H targets (delta_y, delta_phi), at every step -- what tpc_mpc_rollout's target shift leaves when
 *     no new_last_targets is given
 *     x_0 = column k of x0 ([2] rows, leading dimension n), or zeros when x0 is NULL: the reference's case
 * and the loop is tpc_mpc_rollout_newton's on that model, started from no carried controls.
 *   Phase 1, every instance, ONE launch (csrc/mpc_compact_loop.hip; at horizons 4 and 5 the whole loop stays in
 *   registers and no workspace memory is touched).  For k = 0 .. steps-1:
 *     U   <- dlib's shift of the previous step's sequence (mpc.h:231-232: t <- t + 1, the last step kept); zeros at step 0
 *     U   <- clamp(U, lower, upper), then the rounds of tpc_mpc_polish_batch_general at x_k with q->tol, q->max_rounds
 *     verified: u0_k = row 0 of U;  x_{k+1} = A x_k + B u0_k + C in tpc_mpc_rollout's plant arithmetic on the expanded
 *            values, literally: ((A00*x0 + A01*x1) + (B00*u0 + B01*u1)) + C0, the multiplies by 1.0 and 0.0 and the
 *            "+ 0.0" kept (they decide signed zeros and what an Inf becomes);  record u0_k, x_{k+1}, U_k, status = the
 *            rounds used and the two residuals
 *     not verified: the instance stops, first_unverified = k
 *   An instance carried to the end gets first_unverified = steps, and every output row of it equals, bit for bit, what
 *   tpc_mpc_rollout_newton returns on the expanded arrays (the model above, x0 put in, new_last_targets = NULL,
 *   controls_inout = NULL, the same q): controls, states, sequences, status, both residuals and first_unverified.
 *   Phase 2, fallback TPC_MPC_NEWTON_FALLBACK_SOLVE.  The instances with first_unverified < steps and no other flag are
 *   gathered and expanded to the general form on the device (those instances only), run from step 0 through
 *   tpc_mpc_rollout_polished's loop (p's eps / max_iter / smo_iters / algo, the same q) and scattered back: every row of
 *   theirs is what tpc_mpc_rollout_polished returns for exactly those instances in general form, and
 *   TPC_MPC_FLAG_NOT_POLISHED is raised only for (instance, step) pairs that loop leaves at -1.  first_unverified keeps
 *   phase 1's value, so the caller sees who fell back.  The order inside the gathered batch is not defined.  One
 *   4-byte read-back (the number of such instances) sits between the phases.
 *   Fallback TPC_MPC_NEWTON_FALLBACK_NONE.  Phase 1 only: the rows of an unverified instance from first_unverified on
 *   are status -1, zero residuals and zero controls / states / sequences, and the instance raises
 *   TPC_MPC_FLAG_NOT_POLISHED.  With flags_out == NULL and DEVICE memory the call is asynchronous.
 *   Invalid instances (a non-finite v, delta_y, delta_phi or x0; a model value that is not finite; a state that stops
 *   being finite at a later step) behave as in tpc_mpc_rollout_newton: they raise TPC_MPC_FLAG_NONFINITE, stop at that
 *   step (first_unverified = the step, rows as under FALLBACK_NONE), are NOT sent to the fallback under either mode and
 *   do not raise TPC_MPC_FLAG_NOT_POLISHED by themselves.
 * Outputs, SoA with leading dimension n: controls_out [steps*2] (required), states_out [steps*2], sequences_out
 * [steps*H*2] (tpc_mpc_rollout_record's layout: with states_out exactly what tpc_mpc_rollout_backward takes on the
 * expanded arrays), q->status (int32), q->residual_in, q->residual_out [steps], first_unverified (int32) [n]; all but
 * controls_out are optional.  p is validated as tpc_mpc_solve_batch_compact validates it.  A null q, tol <= 0 (or NaN),
 * max_rounds < 0, an unknown fallback, steps < 0 or a dtype other than TPC_MPC_F64 return TPC_MPC_ERR_BAD_ARG.  fp64
 * only, horizons 1..64, two inputs.  n == 0 or steps == 0 returns TPC_MPC_OK with flags 0.  HOST arrays are staged:
 * three (+ 2) rows in, the per-step rows out.
 * A host-only handle (TPC_MPC_DEVICE_NONE) runs FALLBACK_NONE on the calling thread with the kernel's bits (HOST memory
 * only); with FALLBACK_SOLVE it returns TPC_MPC_ERR_NO_DEVICE, after the argument checks above.
 * Not part of this entry: per-instance parameter rows, a caller-given start or controller state in and out, a separate
 * plant or disturbance, a forward-mode kernel of its own (differentiate forward with tpc_mpc_rollout_forward on the
 * expanded arrays at the recorded sequences and states), fp32.  Its backward pass is
 * tpc_mpc_rollout_compact_exact_backward below. */
int tpc_mpc_rollout_compact_exact(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                  const void* delta_y, const void* delta_phi, const void* x0 /* optional [2], ld n */,
                                  int32_t steps, const tpc_mpc_polish* q, int32_t fallback,
                                  void* controls_out /* [steps*2], ld n */, void* states_out /* optional [steps*2] */,
                                  void* sequences_out /* optional [steps*H*2] */,
                                  int32_t* first_unverified /* optional [n] */, uint32_t* flags_out, int mem,
                                  void* stream);

/* The incoming gradient and the outputs of tpc_mpc_rollout_compact_exact_backward, fp64, SoA with leading dimension n.
 * The ten shared parameters are indexed as in tpc_mpc_compact_grad. */
typedef struct tpc_mpc_compact_loop_grad {
    const void *grad_controls;   /* optional [steps*2], ld n: dL/dcontrols_out; NULL = zero */
    const void *grad_states;     /* optional [steps*2], ld n: dL/dstates_out;   NULL = zero */
    void *dv, *ddelta_y, *ddelta_phi;   /* optional outputs [n] */
    void *dx0;                   /* optional output [2], ld n (allowed with x0 == NULL: the gradient at the zero start) */
    void *dparams_rows;          /* optional output [10], ld n */
    void *dparams;               /* optional output [10]: the batch sum */
    void *kkt_residual;          /* optional output [n] */
} tpc_mpc_compact_loop_grad;

/* No reference counterpart.  The backward pass of tpc_mpc_rollout_compact_exact: for n instances that share p's
 * weights, step_size, wheelbase and bounds, the gradient of a loss L(controls_out, states_out) with respect to v,
 * delta_y, delta_phi, x0 and those ten shared parameters, taken at the recorded `sequences` and `states` of that call,
 * without the general form ever being written.
 *   Definition.  Instance k has the expanded model of tpc_mpc_rollout_compact_exact (T = p->step_size, l = p->wheelbase,
 *   Tv = T * v: A = [1, Tv; 0, 1], B = [0, Tv; Tv/l, -Tv/l], C = 0, every target (delta_y, delta_phi) at every step) and
 *   the start x_0 = column k of x0, or (+0.0, +0.0) when x0 is NULL.  The reverse sweep of tpc_mpc_rollout_backward
 *   (csrc/mpc_grad_model.h, rollout_instance<2>, operation for operation, new_last_targets = NULL) runs on that model.
 *   With lambda = 0 and the sums s = 0, for k = steps-1 down to 0, absent gradient arrays counting as +0.0:
 *     mu      = lambda + grad_states[k]
 *     s      += the plant terms of x_{k+1} = A x_k + B u0_k + C (dA += mu x_k', dB += mu u0_k', dC += mu), u0_k = row 0
 *               of sequences[k]
 *     g0[j]   = fma(B[0][j], mu0, fma(B[1][j], mu1, grad_controls[k*2+j]))
 *     qp_step<2>, unchanged, at x_k, U_k = sequences[k] and g = g0 on row 0, 0.0 elsewhere; it adds to s and hands over
 *               dL/dtarget_t = (a_t, b_t) with t from H-1 down to 0.  x_k is x_0 for k = 0, else the recorded
 *               states[k-1]: the state is never recomputed
 *     lambda  = A' mu + dL/dx_k of that solve
 *   Then, every operation rounded on its own:
 *     S = s.A01 + s.B0[1]      D = s.B1[0] - s.B1[1]      Tv = T * v
 *     dv         = T * S + (T / l) * D
 *     ddelta_y   = the sum of every a_t, added to 0.0 one by one in the order they arrive (k descending, t descending
 *                  inside a step); ddelta_phi likewise with b_t
 *     dx0        = lambda after step 0
 *     rows[0..3] = s.Q0, s.Q1, s.R[0], s.R[1]
 *     rows[4]    = v * S + (v / l) * D                               (step_size)
 *     rows[5]    = -((Tv / l) / l) * D                               (wheelbase)
 *     rows[6..9] = s.lo[0], s.lo[1], s.hi[0], s.hi[1]
 *     kkt_residual = s.kkt, the maximum over the steps
 *   dv, dx0, rows and kkt_residual equal, up to the sign of a zero, tpc_mpc_rollout_backward on the expanded arrays
 *   pushed through the same lines; ddelta_y / ddelta_phi are that entry's dtargets rows summed in another order.
 *   dparams[c] is the sum of rows[c] over the contributing instances.
 *   Excluded instances.  A negative entry anywhere in the instance's column of `status` (nobody should differentiate
 *   the zeros that stand in for an unverified step; it raises no flag of its own, and the sweep still runs, so a NaN
 *   speed still raises its flag); a non-finite v, target, x0, recorded state or sequence, incoming gradient or model
 *   value (TPC_MPC_FLAG_NONFINITE); a model that breaks dlib's requires clause (TPC_MPC_FLAG_BAD_MODEL).  An excluded
 *   instance gets 0.0 in every per-instance output and adds nothing to dparams.
 *   Method.  One lane per instance (csrc/mpc_compact_loop_grad.hip); lambda, the sums and the two target sums stay in
 *   registers over the steps, one step's values live in the handle's gradient workspace and are reused by every step,
 *   at horizons 4 and 5 in registers.  dparams is summed as tpc_mpc_solve_batch_compact_exact_backward sums it -- no
 *   floating-point atomics, the same bytes on every call; the order depends on n and is not the ascending-k order.
 * p is validated as tpc_mpc_solve_batch_compact validates it.  v, delta_y, delta_phi [n], sequences ([steps*H*2]) and
 * states ([steps*2]) as tpc_mpc_rollout_compact_exact returned them are required; x0 ([2]) and status (int32 [steps],
 * q->status of that call) are optional; every output of g is optional, and with none the call only sets the flags.
 * fp64 only, horizons 1..64.  A null g, null sequences or states, steps < 0 or a dtype other than TPC_MPC_F64 return
 * TPC_MPC_ERR_BAD_ARG.  n == 0 or steps == 0 returns TPC_MPC_OK with flags 0 and writes zeros to dparams.  HOST arrays
 * are staged; with DEVICE memory and flags_out == NULL the call is asynchronous on `stream`.  A host-only handle
 * (TPC_MPC_DEVICE_NONE) runs HOST batches on the calling thread with the kernel's per-instance bits, its dparams summed
 * in ascending k, and returns TPC_MPC_ERR_NO_DEVICE for DEVICE memory.
 * Not part of this entry: forward mode, per-instance parameter rows, a separate plant or disturbance, fp32. */
int tpc_mpc_rollout_compact_exact_backward(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, const void* v,
                                           const void* delta_y, const void* delta_phi,
                                           const void* x0 /* optional [2], ld n */, int32_t steps,
                                           const void* sequences /* [steps*H*2] */, const void* states /* [steps*2] */,
                                           const int32_t* status /* optional [steps], ld n */,
                                           const tpc_mpc_compact_loop_grad* g, uint32_t* flags_out, int mem,
                                           void* stream);

/* Inputs and outputs of tpc_mpc_rollout_backward, SoA with the io's leading dimension ld:
 *   sequences[steps*H*I]  the recorded sequences, as tpc_mpc_rollout_record returns them (required)
 *   states[steps*2]       the recorded states_out of the same call (required)
 *   grad_controls[steps*I], grad_states[steps*2]
 *                         dL/dcontrols_out, dL/dstates_out; optional, NULL = zero
 *   dA[4] dB[2*I] dC[2] dQ[2] dR[I] dlower[I] dupper[I] dx0[2] dtargets[H*2]
 *                         optional outputs, dL/d(the io array of the same name and shape); overwritten; NULL = not computed
 *   dnew_last_targets[steps*2]  optional output, dL/dnew_last_targets (row 0, never read by the rollout, is 0)
 *   kkt_residual[1]       optional output: max over the steps of the single solve's residual */
typedef struct tpc_mpc_rollout_grad {
    const void *sequences, *states, *grad_controls, *grad_states;
    void *dA, *dB, *dC, *dQ, *dR, *dlower, *dupper, *dx0, *dtargets, *dnew_last_targets;
    void* kkt_residual;
} tpc_mpc_rollout_grad;

/* No reference counterpart.  The backward pass of tpc_mpc_rollout (the closed loop of test/mpc.cpp:301-316): for n
 * instances, the gradient of a loss L(controls_out, states_out) with respect to every model input, the initial state,
 * the initial targets and new_last_targets.
 *   Definition.  S = steps.  x_0 = io->x0; step k solves from x_k with the targets T_k and returns U_k (its row 0 is
 *   u0_k = controls_out[k]); x_{k+1} = A x_k + B u0_k + C = states_out[k].  The target shift of operator()
 *   (mpc.h:236-237) and set_last_target give T_k[t] = targets[t+k] for t + k <= H-1, else, with m = t + k - (H-1),
 *   new_last_targets[m] (targets[H-1] when new_last_targets is NULL).  Each step is differentiated as
 *   tpc_mpc_solve_batch_general_backward defines it (active set read off U_k, the free components at the stationary
 *   point); the warm start (controls_inout, v_inout) gets no gradient.  x_k for k >= 1 is read from `states`, not
 *   recomputed, so the derivative is taken at the forward's bits.
 *   Method.  One reverse sweep per instance, lambda = 0:
 *     for k = S-1 .. 0:  mu = lambda + dL/dstates_out[k];  dA += mu x_k', dB += mu u0_k', dC += mu;
 *                        the single-solve backward of step k with dL/dU_k = (dL/dcontrols_out[k] + B' mu) on row 0,
 *                        0 elsewhere, which adds to dA .. dupper, gives dL/dT_k (added into dtargets /
 *                        dnew_last_targets through the map above) and dL/dx_k of the solve, d;
 *                        lambda = A' mu + d
 *     dx0 = lambda;  kkt_residual = max over the steps.
 *   One lane per instance runs the whole sweep in one launch; lambda and the sums stay in registers, the per-step
 *   Riccati workspace of the handle (slots * H doubles per instance) is reused by every step.
 * io, p, steps and new_last_targets: as for the tpc_mpc_rollout call that recorded sequences and states (io's
 * controls_inout, v_inout, u0 and iters are ignored).  fp64 only, horizons 1..64, one or two inputs.
 * dnew_last_targets without new_last_targets is TPC_MPC_ERR_BAD_ARG.  Flags, memory, stream and the host-only
 * handle as tpc_mpc_solve_batch_general_backward: an instance with non-finite data, sequences, states or gradients
 * (TPC_MPC_FLAG_NONFINITE) or a model that breaks dlib's requires clause (TPC_MPC_FLAG_BAD_MODEL) gets all-zero
 * outputs. */
int tpc_mpc_rollout_backward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                             int32_t steps, const void* new_last_targets, const tpc_mpc_rollout_grad* g,
                             uint32_t* flags_out, int mem, void* stream);

/* K directions of tpc_mpc_solve_batch_general_forward / tpc_mpc_rollout_forward.  A direction is a tangent of every
 * input: tA[4] tB[2*I] tC[2] tQ[2] tR[I] tlower[I] tupper[I] tx0[2] ttargets[H*2] tnew_last_targets[steps*2], each the
 * tangent of the array of the same name and shape.  Every array is optional (NULL = zero) and holds the K directions as
 * K stacked row blocks, SoA with the io's ld: element (d, c, k) of a C-component array is base[(d*C + c)*ld + k]. */
typedef struct tpc_mpc_tangents {
    int32_t directions, reserved;
    const void *tA, *tB, *tC, *tQ, *tR, *tlower, *tupper, *tx0, *ttargets, *tnew_last_targets;
} tpc_mpc_tangents;

/* No reference counterpart.  Forward mode (Jacobian-vector products) of tpc_mpc_solve_batch_general: for n instances and
 * K directions, the directional derivative tcontrols[K*H*I] of the controls u along each direction, given u.
 *   Definition.  Notation and active set as tpc_mpc_solve_batch_general_backward: component (t, j) is ACTIVE iff
 *   u <= lower_j || u >= upper_j, the u <= lower_j test first; F is the rest.  x_k below is io->x0 and tx_k is tx0.
 *     ub(t,j)  = tlower_j / tupper_j on an active component (by the bound it sits on), 0 on F
 *     forward  t = 0..H-1 : x_{t+1}  = A x_t + B u_t + C                            (x_0 = x_k)
 *                           tx_{t+1} = tA x_t + A tx_t + tB u_t + B ub_t + tC       (tx_0 = tx_k)
 *     backward t = H-1..0 : e   = x_{t+1} - T[t]
 *                           p_t  = A' p_{t+1} + Q e
 *                           tp_t = tA' p_{t+1} + A' tp_{t+1} + tQ e + Q (tx_{t+1} - tT[t])
 *                           r_t  = tB' p_t + B' tp_t + tR u_t + R ub_t
 *                           masked Riccati step with g = r_t, F as above (the arithmetic of the backward pass)
 *     tU = ub - w,  w = H_FF^-1 r_F (w = 0 off F)
 *   r is the directional derivative of dlib's df = H u + MM along (the direction, ub), taken at u, so tU is the
 *   derivative of the map tpc_mpc_solve_batch_general_backward differentiates, and the linear map direction -> tU is,
 *   operation by operation, the transpose of what that entry computes:  sum G . tU = sum_theta <dL/dtheta, ttheta> for
 *   every G = dL/du, to rounding.  When u is the optimum it is the derivative of the optimum.
 *   Method.  One lane per (direction, instance) pair, lane L = direction L / n of instance L % n, all K directions in
 *   one launch (csrc/mpc_tangent_model.h): a forward pass, the fused costate / Riccati pass, and the forward pass that
 *   turns gains into w.  The per-step quantities live in device scratch of the handle.
 * controls [H*I] (required) is u; t (required) the directions, 1 <= t->directions and directions * n < 2^31
 * (TPC_MPC_ERR_BAD_ARG otherwise); t->tnew_last_targets is ignored.  tcontrols (required): element (d, c, k) at
 * tcontrols[(d*H*I + c)*ld + k].  io, p: as for tpc_mpc_solve_batch_general_backward; fp64 only, horizons 1..64, one or
 * two inputs.  An instance with non-finite data or controls, or tangents in direction d (the bounds' tangents must be
 * finite; the bounds may be infinite), raises TPC_MPC_FLAG_NONFINITE, a model that breaks dlib's requires clause
 * TPC_MPC_FLAG_BAD_MODEL; that (d, k) pair gets an all-zero block.  n == 0 returns TPC_MPC_OK with flags 0.  Memory,
 * stream, flags and the host-only handle as tpc_mpc_solve_batch_general_backward. */
int tpc_mpc_solve_batch_general_forward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                        const void* controls, const tpc_mpc_tangents* t, void* tcontrols,
                                        uint32_t* flags_out, int mem, void* stream);

/* No reference counterpart.  Forward mode of tpc_mpc_rollout: for n instances and K directions, the directional
 * derivatives of (controls_out, states_out) of the closed loop, taken at the recorded sequences and states.  With few
 * parameters and many outputs (a Jacobian for Gauss-Newton / Levenberg-Marquardt, a sensitivity study) it replaces one
 * tpc_mpc_rollout_backward call per output by one direction per parameter, all of them in one launch.
 *   Definition.  Notation as tpc_mpc_rollout_backward: step k solves from x_k (io->x0 for k = 0, states[k-1] after) with
 *   the shifted targets T_k and has the recorded sequence U_k; tT_k[t] comes from ttargets / tnew_last_targets through
 *   the same map as T_k.  The tangent of step k is the step of tpc_mpc_solve_batch_general_forward at (x_k, tx_k, T_k,
 *   tT_k, U_k); only its row 0 feeds the plant:
 *     tu0_k    = ub_0 - k_0          the Riccati response starts at dx_0 = 0, so w_0 is the sweep's feed-forward k_0 at
 *                                    t = 0: one forward and one fused backward pass per step, no stored gains
 *     tx_{k+1} = tA x_k + A tx_k + tB u0_k + B tu0_k + tC                     (tx_0 = tx0)
 *     tcontrols[k] = tu0_k,  tstates[k] = tx_{k+1}
 *   The map direction -> (tcontrols, tstates) is, operation by operation, the transpose of tpc_mpc_rollout_backward:
 *   sum G_u . tcontrols + sum G_x . tstates = sum_theta <dL/dtheta, ttheta>, to rounding.  When every U_k is the optimum
 *   (tpc_mpc_rollout_polished, tpc_mpc_rollout_newton) it is the derivative of the closed loop; the warm start gets no
 *   tangent, as it gets no gradient.
 *   Method.  One lane per (direction, instance) pair as in tpc_mpc_solve_batch_general_forward, every step and every
 *   direction in one launch (csrc/mpc_rollout_tangent.hip); tx_k stays in registers from step to step.
 * io, p, steps, new_last_targets, sequences [steps*H*I] and states [steps*2] (both required): as for
 * tpc_mpc_rollout_backward.  t (required): 1 <= t->directions, directions * n < 2^31; tnew_last_targets without
 * new_last_targets is TPC_MPC_ERR_BAD_ARG.  tcontrols (required): element (d, c, k) at tcontrols[(d*steps*I + c)*ld + k];
 * tstates (optional): [(d*steps*2 + c)*ld + k].  fp64 only, horizons 1..64, one or two inputs.  n == 0 or steps == 0
 * returns TPC_MPC_OK with flags 0.  Flags, zeroed (d, k) blocks, memory, stream and the host-only handle as
 * tpc_mpc_solve_batch_general_forward (non-finite sequences or states count as non-finite data). */
int tpc_mpc_rollout_forward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io, int32_t steps,
                            const void* new_last_targets, const void* sequences, const void* states,
                            const tpc_mpc_tangents* t, void* tcontrols, void* tstates, uint32_t* flags_out, int mem,
                            void* stream);

/* ---- closed loops against a separate plant ------------------------------------------------------ */

/* The closed loops above move the state with the controller's own model.  A plant is what moves it instead: three
 * optional arrays and an optional disturbance, nothing else.  Every pointer null is the controller's model and no
 * disturbance: the parent loop, bit for bit, signed zeros included. */
typedef struct tpc_mpc_plant {
    const void *A, *B, *C;      /* [4] [2*I] [2], SoA with the io's ld; all three or none (none = the controller's) */
    const void *disturbance;    /* optional, [steps*2], SoA with leading dimension ld_d; row k is added to x_{k+1}   */
    int64_t ld_d;
} tpc_mpc_plant;

#define TPC_MPC_LOOP_RECORD 0     /* tpc_mpc_rollout_record   */
#define TPC_MPC_LOOP_POLISHED 1   /* tpc_mpc_rollout_polished */
#define TPC_MPC_LOOP_NEWTON 2     /* tpc_mpc_rollout_newton   */
/* The closed loop `loop` against a separate plant, fp64 only.
 *   Definition.  Step k is the named parent's step -- the solve / polish / Newton rounds at x_k with the controller's
 *   A, B, C, Q, R, bounds and T_k -- except its last line, which becomes
 *     x_{k+1} = ((Ap x_k + Bp u0_k) + Cp) (+ d_k)
 *   in the step tail's arithmetic, operation for operation (no fused multiply-add, the same association); the
 *   disturbance's row k is one more plain add at the end, and no add at all when plant->disturbance is null.
 * plant (required; its A, B, C all given or all null, one or two of them is TPC_MPC_ERR_BAD_ARG): any finite Ap, Bp,
 * Cp, d is allowed, there is no requires clause.  TPC_MPC_LOOP_NEWTON: an instance with a non-finite plant or
 * disturbance value raises TPC_MPC_FLAG_NONFINITE and is left as tpc_mpc_rollout_newton leaves an instance with a
 * non-finite model (first_unverified 0, status -1 and zeros from step 0, not handed to the fallback).  The solve-based
 * loops carry such a value into x_{k+1}, where the next step's solve raises the flag as for a non-finite x0.
 * Arguments the chosen loop does not have are ignored (q, fallback, first_unverified for _RECORD; fallback,
 * first_unverified for _POLISHED); every other argument and check is the parent's, an unknown loop is
 * TPC_MPC_ERR_BAD_ARG.  A host-only handle runs TPC_MPC_LOOP_NEWTON with TPC_MPC_NEWTON_FALLBACK_NONE on the calling
 * thread with the kernel's bits; anything else is TPC_MPC_ERR_NO_DEVICE, reported after the argument checks. */
int tpc_mpc_rollout_plant(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                          const tpc_mpc_plant* plant, int32_t loop, int32_t steps, const void* new_last_targets,
                          const tpc_mpc_polish* q, int32_t fallback, void* controls_out, void* states_out,
                          int32_t* iters_out, void* sequences_out, int32_t* first_unverified, uint32_t* flags_out,
                          int mem, void* stream);

/* Gradients of the plant's inputs: [4] [2*I] [2] with the io's ld, ddisturbance [steps*2] with the plant's ld_d (the
 * io's ld when the plant has no disturbance).  All optional, all overwritten. */
typedef struct tpc_mpc_plant_grad {
    void *dA, *dB, *dC, *ddisturbance;
} tpc_mpc_plant_grad;
/* tpc_mpc_rollout_backward against a separate plant.  The sweep, for k = steps-1 .. 0 with lambda = 0 at the end:
 *     mu = lambda + G_x[k]
 *     dAp += mu x_k',  dBp += mu u0_k',  dCp += mu,  ddisturbance[k] = mu
 *     dL/du0_k = G_u[k] + Bp' mu
 *     lambda = Ap' mu + d          (d: the solve's dL/dx_k)
 * and the controller's dA .. dupper receive the solves' contributions only.  With the plant's arrays null the plant
 * terms go into dA, dB, dC as in tpc_mpc_rollout_backward (pg's dA, dB, dC must then be null: TPC_MPC_ERR_BAD_ARG);
 * ddisturbance may be asked for without a disturbance: it is the gradient at d = 0.  The disturbance itself is not
 * read (the states are recorded).  plant and pg are required; everything else as tpc_mpc_rollout_backward, non-finite
 * plant values counting as non-finite data. */
int tpc_mpc_rollout_plant_backward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                   const tpc_mpc_plant* plant, int32_t steps, const void* new_last_targets,
                                   const tpc_mpc_rollout_grad* g, const tpc_mpc_plant_grad* pg, uint32_t* flags_out,
                                   int mem, void* stream);

/* Tangents of the plant's inputs, K = t->directions stacked row blocks like tpc_mpc_tangents' (element (d, c, k) of a
 * C-component array at base[(d*C + c)*ld + k]; tdisturbance [K*steps*2] with the plant's ld_d).  Null = zero. */
typedef struct tpc_mpc_plant_tangents {
    const void *tA, *tB, *tC, *tdisturbance;
} tpc_mpc_plant_tangents;
/* tpc_mpc_rollout_forward against a separate plant:
 *     tx_{k+1} = tAp x_k + Ap tx_k + tBp u0_k + Bp tu0_k + tCp + td_k
 * and t's tA, tB, tC enter the step's QP only.  With the plant's arrays null the controller's model and its tangents
 * move the state as in tpc_mpc_rollout_forward (pt's tA, tB, tC must then be null).  The transpose identity of
 * tpc_mpc_rollout_forward holds with the plant's and the disturbance's terms on its right-hand side.  plant is
 * required, pt may be null (all zero); everything else as tpc_mpc_rollout_forward. */
int tpc_mpc_rollout_plant_forward(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_general_io* io,
                                  const tpc_mpc_plant* plant, int32_t steps, const void* new_last_targets,
                                  const void* sequences, const void* states, const tpc_mpc_tangents* t,
                                  const tpc_mpc_plant_tangents* pt, void* tcontrols, void* tstates,
                                  uint32_t* flags_out, int mem, void* stream);

/* ---- batched cycle(): raw trajectories in, CarCommand fields out -------------------------------- */

/* Polylines of n instances, SoA: point i of instance k at base[i*ld + k] (float), `count[k]` points
 * used (<= max_points).  Fields of street_environment::TrajectoryPoint the module reads:
 * position.x/y, directory.x/y, velocity. */
typedef struct tpc_mpc_trajectories {
    int64_t n, ld;
    int32_t max_points, reserved;
    const float *pos_x, *pos_y, *dir_x, *dir_y, *velocity;
    const int32_t* count;
    const float* car_velocity;   /* car->velocity()                                    (follower.cpp:78)  */
    const float* look_ahead;     /* distanceToTrajectoryPoint after the lookup/FOH rule (follower.cpp:66-73) */
} tpc_mpc_trajectories;

/* Replaces, for n independent controllers in DEVICE memory, the tobiMPC branch of cycle():
 * getTrajectoryPoint (src/trajectory_point_follower.cpp:392-443, without the stateful crossing-stop
 * PID of :445-473), the speed clamp and target extraction (:78-85), the velocity lookup (:323;
 * lookup_x/lookup_y of lookup_n entries, ascending x, piecewise linear, clamped; lookup_n = 0 keeps
 * the speed), mpcControllerTobi (:97) and the crossing rule (:277-283: targetSpeed < 0.5 zeroes the
 * steering).  Outputs: steering_front/rear (double), target_speed, target_distance (float;
 * CarCommand::State fields of :114-117).  fp64 solve; uses p's compact-model fields. */
int tpc_mpc_follow_batch(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_trajectories* t,
                         const float* lookup_x, const float* lookup_y, int32_t lookup_n,
                         double* steering_front, double* steering_rear, float* target_speed,
                         float* target_distance, int32_t* iters, uint32_t* flags_out, void* stream);

/* The same with ONE TRAJECTORY POINT PER HORIZON STEP: step t of the horizon gets the target
 * (position.y, atan2(directory)) of the polyline point at arc length look_ahead + t * spacing, fed
 * through dlib::mpc::set_target(val, t) semantics (mpc.h:142-155) to the general-form solver; the
 * model, weights and bounds are the compact ones (p).  spacing = step_spacing[k] (float, optional) or,
 * when NULL, |v| * step_size -- the distance driven per step; a negative step_spacing[k] is taken as it is
 * (the arc lengths shrink with t, each step's point is the one getTrajectoryPoint returns for its arc
 * length; such an instance walks its polyline once per step).  Step 0 is tpc_mpc_follow_batch's point,
 * so target_speed / target_distance and the crossing rule are the same; with spacing 0 the whole
 * call equals tpc_mpc_follow_batch.  targets_out (optional, double, SoA [2N][n]) receives the targets
 * used.  The reference module itself sets one target for all steps (src/...follower.cpp:368-371):
 * this is the SURVEY.md 8f-1 extension, its geometry "parity unpinned" like tpc_mpc_follow_batch's. */
int tpc_mpc_follow_batch_horizon(tpc_mpc_handle h, const tpc_mpc_params* p, const tpc_mpc_trajectories* t,
                                 const float* step_spacing, const float* lookup_x, const float* lookup_y,
                                 int32_t lookup_n, double* steering_front, double* steering_rear,
                                 float* target_speed, float* target_distance, double* targets_out,
                                 int32_t* iters, uint32_t* flags_out, void* stream);

/* ---- sharding a batch over the GPUs of a node ---------------------------------------------------- */

/* No reference counterpart (the reference solves one problem per cycle on one CPU thread).  Instances
 * are independent, so a batch shards over GPUs with no exchange during the solve; the one collective
 * is an all-gather of the control outputs over RCCL/xGMI.  One handle per GPU; the handles of a job
 * (one per process, or several in one process) form a communicator the NCCL way: rank 0 obtains an
 * id, the host distributes it, every rank calls tpc_mpc_comm_init_rank.  A handle without a
 * communicator is a world of one.  RCCL is loaded on first use (dlopen); TPC_MPC_ERR_COMM if absent. */
#define TPC_MPC_COMM_ID_BYTES 128
int tpc_mpc_comm_unique_id(void* id, size_t len);
int tpc_mpc_comm_init_rank(tpc_mpc_handle h, const void* id, size_t len, int rank, int world);
int tpc_mpc_comm_destroy(tpc_mpc_handle h);
/* TEST HOOK, not for hosts: a world of one normally needs no communicator and the exchange is skipped.
 * force_communicator != 0 makes the next tpc_mpc_comm_init_rank(h, id, len, 0, 1) build a real one-rank RCCL
 * communicator, so that a one-GPU box runs the library's own ncclAllGather calls; force_ragged != 0 makes the
 * sharded solve take its ragged form (one in-place ncclBroadcast per owner) whatever the sizes. */
int tpc_mpc_comm_test_mode(tpc_mpc_handle h, int force_communicator, int force_ragged);
/* ncclGroupStart / ncclGroupEnd: a single thread that drives several handles brackets its
 * tpc_mpc_comm_init_rank calls, and each round of tpc_mpc_solve_batch_compact_sharded calls, with these. */
int tpc_mpc_group_begin(void);
int tpc_mpc_group_end(void);
/* The contiguous block of a batch of n_total that `rank` of `world` owns (blocks differ by <= 1). */
int tpc_mpc_shard_range(int64_t n_total, int rank, int world, int64_t* first, int64_t* count);
/* How a batch is split over the ranks (ABI 5).  BLOCK: rank r owns one contiguous block (tpc_mpc_shard_range).
 * INTERLEAVED: rank r owns the instances i = r (mod world).  The iteration count of an instance is a function of its
 * speed (dlib's lambda, mpc.h:116-123), so a batch that arrives SORTED by speed gives one rank of a block split all the
 * 10 000-iteration instances; the interleaved split deals them round.  For iid inputs the two cost the same.
 * tpc_mpc_shard_map: element j of rank's shard is instance first + j * stride, j < count. */
#define TPC_MPC_SPLIT_BLOCK 0
#define TPC_MPC_SPLIT_INTERLEAVED 1
int tpc_mpc_shard_map(int64_t n_total, int rank, int world, int split, int64_t* first, int64_t* count, int64_t* stride);

/* tpc_mpc_solve_batch_compact for this rank's block of a batch of n_total, then the all-gather:
 * v/delta_y/delta_phi_shard hold the block's `count` instances, steering_front_all / _rear_all are
 * FULL-size arrays [n_total]; the block is solved straight into its slot [first, first+count) and the
 * slots are exchanged in place (ncclAllGather when n_total divides evenly, otherwise one in-place
 * ncclBroadcast per owner inside one group), so on return -- in stream order -- every GPU holds all
 * control outputs.  DEVICE memory only; iters_shard [count] and flags_out cover this rank's block. */
int tpc_mpc_solve_batch_compact_sharded(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n_total,
                                        const void* v_shard, const void* delta_y_shard,
                                        const void* delta_phi_shard, void* steering_front_all,
                                        void* steering_rear_all, int32_t* iters_shard,
                                        uint32_t* flags_out, void* stream);

/* The same with the split named (ABI 5).  TPC_MPC_SPLIT_BLOCK: exactly the call above.  TPC_MPC_SPLIT_INTERLEAVED: the shard
 * arrays hold the rank's `count` instances compacted (element j = instance rank + j * world: the host scatters with a
 * stride); the shard is solved into the rank's slot of a [world][ceil(n_total / world)] staging array owned by the
 * handle, the slots are all-gathered there (equal sizes by construction: one ncclAllGather per output, no ragged form)
 * and one kernel per output writes them back in INSTANCE order, so the full-size outputs look the same under either
 * split -- bit for bit within one kernel family.  iters_shard [count] stays in shard order. */
int tpc_mpc_solve_batch_compact_sharded_split(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n_total, int split,
                                              const void* v_shard, const void* delta_y_shard,
                                              const void* delta_phi_shard, void* steering_front_all,
                                              void* steering_rear_all, int32_t* iters_shard,
                                              uint32_t* flags_out, void* stream);

/* No reference counterpart (the reference drives one dlib::mpc object on one device: src/trajectory_point_follower.cpp:366).
 * The general form sharded the same way: io_all describes the FULL batch (n = n_total, ld >= n_total, DEVICE memory;
 * every rank passes the same shapes).  The rank solves columns [first, first + count) of those arrays in place -- only
 * that block of the inputs has to be filled on this rank -- and the I rows of u0 are exchanged in place as above, so on
 * return every GPU holds all of u0.  controls_inout / v_inout / iters, when given, are read and written for this
 * rank's block only and not exchanged; flags_out covers this rank's block. */
int tpc_mpc_solve_batch_general_sharded(tpc_mpc_handle h, const tpc_mpc_params* p,
                                        const tpc_mpc_general_io* io_all, uint32_t* flags_out, void* stream);

/* No reference counterpart.  The exchange of the two calls above by itself, for every OTHER entry point a host wants
 * to shard (tpc_mpc_solve_batch_compact_mixed, tpc_mpc_follow_batch*, tpc_mpc_rollout, ...): each rank calls that entry
 * for its block -- tpc_mpc_shard_range says which -- with output pointers offset to the block's slot [first, first + count)
 * of FULL-size arrays, then this.  rows[i] (i < n_rows) is the DEVICE base of one full-size output row of n_total
 * elements of elem_bytes (4 or 8) each; on return -- in stream order -- every GPU holds every rank's slot of every row
 * (ncclAllGather when n_total divides evenly, otherwise one in-place ncclBroadcast per owner; one RCCL group).  A handle
 * without a communicator: a no-op. */
int tpc_mpc_gather_shards(tpc_mpc_handle h, int64_t n_total, void* const* rows, int n_rows, int elem_bytes, void* stream);
/* The same with the split named (ABI 5).  TPC_MPC_SPLIT_INTERLEAVED: on entry the FIRST `count` elements of each row are
 * this rank's shard (element j = instance rank + j * world -- what an entry called on the compacted shard leaves when its
 * output pointer is the row's base); on return the row holds all n_total elements in instance order. */
int tpc_mpc_gather_shards_split(tpc_mpc_handle h, int64_t n_total, int split, void* const* rows, int n_rows, int elem_bytes,
                                void* stream);

/* ---- memory ------------------------------------------------------------------------------------ */

/* No reference counterpart.  A handle grows its device scratch on demand, and growing frees and
 * allocates device memory, which synchronises the whole device; a host that keeps several batches
 * in flight (one handle and one stream per batch) calls this once per handle up front for the
 * largest compact batch it will solve (mem: where the batch arrays will live), so that no solve
 * allocates. */
int tpc_mpc_reserve(tpc_mpc_handle h, const tpc_mpc_params* p, int64_t n, int mem);

/* ---- library options -------------------------------------------------------------------------- */

/* No reference counterpart: switches of this implementation that a host may want to pin (A/B measurements,
 * boards without a large BAR).  They belong to the handle -- the library reads nothing from the environment.
 *   TPC_MPC_OPT_WAVE_GROUP   instances per wavefront of the fp64 WAVE kernels: 0 (default) = as many as fit and
 *                            pay (4 with inputs*horizon <= 16, 2 with <= 32, from one wavefront per SIMD on),
 *                            1 = strictly one, 2 / 4 = pairs / fours where they fit.  Same arithmetic per instance.
 *   TPC_MPC_OPT_MAILBOX_HOST 1 = tpc_mpc_solve_one's request lines live in pinned host memory even where the
 *                            CPU could write device memory through the BAR (0, default: device memory where
 *                            hipDeviceAttributeIsLargeBar says so).  Restarts the resident wavefront (the idle
 *                            timeout and "resident off" of tpc_mpc_set_resident are kept).
 *   TPC_MPC_OPT_GROUP_LANES  lanes per instance of the GROUP family: 0 (default) = the measured best for the batch
 *                            size (csrc/auto_table.h), 2 / 4 / 8 where that size is built for the horizon (N = 10:
 *                            2, 4; N = 20, 30, 40: 2, 4, 8).
 *   TPC_MPC_OPT_HOST_SOLVE_ONE  tpc_mpc_solve_one on the CALLING THREAD for horizons up to this value (0, default:
 *                            never): the host path of csrc/tpc_mpc_host.cpp, as on a handle created with
 *                            TPC_MPC_DEVICE_NONE.  For a module that solves one short-horizon problem per cycle --
 *                            the reference's own N = 4 -- set it to 10: a core needs ~4 us at N = 4 (28 at N = 10) where the
 *                            round trip to the resident wavefront needs ~10 (30); from N = 20 on the GPU is faster
 *                            (INTEGRATION.md section 1). */
typedef enum tpc_mpc_option { TPC_MPC_OPT_WAVE_GROUP = 1, TPC_MPC_OPT_MAILBOX_HOST = 2, TPC_MPC_OPT_GROUP_LANES = 3,
                              TPC_MPC_OPT_HOST_SOLVE_ONE = 4 } tpc_mpc_option;
int tpc_mpc_set_option(tpc_mpc_handle h, int option, int64_t value);

/* ---- measurement ------------------------------------------------------------------------------ */

/* No reference counterpart (the reference times nothing on this branch; its only timers are
 * logger.time("mikMPC") around the other back-end, src/trajectory_point_follower.cpp:134,213).
 * With profiling on, every solve records HIP events on its launch stream around each kernel;
 * tpc_mpc_last_kernel_times waits for the last solve and returns the two kernel durations in ms
 * (LANE: coordinate-descent kernel, projected-gradient kernel; WAVE: the one kernel, 0) and the
 * tpc_mpc_algo that ran. */
int tpc_mpc_set_profiling(tpc_mpc_handle h, int enable);
int tpc_mpc_last_kernel_times(tpc_mpc_handle h, double* first_ms, double* second_ms, int* algo);

/* Occupancy statistics of the last LANE solve (waits for that solve): loop iterations executed
 * by all persistent wavefronts of the projected-gradient kernel, and refill blocks executed.
 * lane utilisation = sum of per-instance PG iterations / (64 * wave_iterations). */
int tpc_mpc_last_lane_stats(tpc_mpc_handle h, uint64_t* wave_iterations, uint64_t* refill_blocks);

#ifdef __cplusplus
}
#endif
#endif /* TPC_MPC_H */
