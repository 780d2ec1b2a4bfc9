"""torch autograd over MpcSolver's batched entries.  Inputs are CUDA fp64 tensors, component-major
(solve_batch_general's layout); every function is once-differentiable; forward mode is torch.autograd.forward_ad, one
direction per dual level, taken at the same sequences the backward is taken at; torch.func transforms are not
supported.  include/tpc_mpc.h defines the derivative: the active set is read off the solved sequence and the free
components are differentiated through the stationarity condition on that set, so it is the gradient of the optimum when
the sequence is the optimum -- dlib's default eps 0.01 leaves a loose one: pass polish=True (a Newton round or two onto
the verified optimum, the cheap way) or a small eps (e.g. eps=1e-10).  Instances whose data are non-finite or break
dlib's requires clause get zero gradients.  All launches go to torch's current stream.

mpc_general          the solved sequence of n fresh controllers.
    forward   MpcSolver.solve_batch_general from zero controls, then polish_batch_general with polish
    backward  tpc_mpc_solve_batch_general_backward
    jvp       tpc_mpc_solve_batch_general_forward
    saved     the nine arrays and the controls
mpc_compact          the reference controller, (front, rear): compact_general_form, then mpc_general.
    forward, backward, jvp, saved: mpc_general's; torch's chain rule carries them through the expansion
mpc_rollout          the closed loop of n fresh controllers, optionally against a separate plant.
    forward   MpcSolver.rollout_record; rollout_polished with polish, rollout_newton with newton_first
    backward  tpc_mpc_rollout_backward (tpc_mpc_rollout_plant_backward with a plant or a disturbance)
    jvp       tpc_mpc_rollout_forward (tpc_mpc_rollout_plant_forward)
    saved     the nine arrays, the five optional ones (None where not given), the states and every step's sequence
mpc_compact_exact    the reference controller at the verified optimum, shared or per-instance parameters.
    forward   MpcSolver.solve_batch_compact_exact (the rows entry with a per-instance parameter), no general form
    backward  tpc_mpc_solve_batch_compact_exact_backward (_rows_backward)
    jvp       tpc_mpc_solve_batch_compact_exact_forward
    saved     v, delta_y, delta_phi, the [10, n] rows if any, the sequence and the status
mpc_rollout_compact  the reference controller's closed loop, every step the verified optimum.
    forward   MpcSolver.rollout_compact_exact, no general form
    backward  "expanded": tpc_mpc_rollout_backward on compact_general_form, built in the backward only;
              "fused": tpc_mpc_rollout_compact_exact_backward, no general form
    jvp       none
    saved     v, delta_y, delta_phi, the states, every step's sequence and x0 (None where not given)
compact_general_form is the one place the reference controller's model is expanded to the general form.
"""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

_ALPHA_MAX = 22.0 * math.pi / 180.0   # the reference module's steering bounds

MODEL_NAMES = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets")       # solve_batch_general's order
_ROLLOUT_NAMES = MODEL_NAMES + ("new_last_targets", "Ap", "Bp", "Cp", "disturbance")   # the last five optional
_COMPACT_NAMES = ("v", "delta_y", "delta_phi")
# the ten compact parameters as the five arguments that carry them: (name, shared shape, where in the ten), in the
# order of COMPACT_PARAM_NAMES
_COMPACT_PARAMS = (("weights", (4,), slice(0, 4)), ("step_size", (), 4), ("wheelbase", (), 5),
                   ("lower", (2,), slice(6, 8)), ("upper", (2,), slice(8, 10)))
_WEIGHT_KEYS = ("weight_y", "weight_phi", "weight_steering_front", "weight_steering_rear")
_BY_VALUE = _WEIGHT_KEYS + ("step_size", "wheelbase", "lower", "upper")   # tpc_mpc_params' fields of the ten


def _require_cuda_f64(message, *tensors):
    for t in tensors:
        if t is not None and not (t.is_cuda and t.dtype == torch.float64):
            raise ValueError(message)


def _polish(polish):
    """(tol, max_rounds) of a polish argument that is on: True is (1e-9, 8)"""
    return (1e-9, 8) if polish is True else tuple(polish)


def _contiguous(g):
    return None if g is None else g.contiguous()


def _parse_params(over, params, n=None):
    """The five parameter arguments (in _COMPACT_PARAMS' order, None: the solver's value) -> (over, given, rows): the
    given ones as tensors, shapes checked.  rows: with n, whether the call is a per-instance one -- only a tensor one
    dimension longer than the shared shape makes it one (`weights` [4] at n == 4 is shared); a parameter may then be
    [..., n], a CUDA fp64 tensor.  Otherwise the values go into a copy of `over`, as tpc_mpc_params takes them."""
    over, given = dict(over), []
    rows = n is not None and any(torch.is_tensor(t) and t.dim() == len(shape) + 1
                                 for (_, shape, _), t in zip(_COMPACT_PARAMS, params))
    for (name, shape, _), t in zip(_COMPACT_PARAMS, params):
        if t is not None:
            t = t if torch.is_tensor(t) else torch.as_tensor(t, dtype=torch.float64)
            if rows and tuple(t.shape) == shape + (n,):
                _require_cuda_f64(f"per-instance {name} must be a CUDA fp64 tensor", t)
            elif tuple(t.shape) != shape:
                either = f" or {list(shape + (n,))}" if rows else ""
                raise ValueError(f"{name} must have shape {list(shape)}{either}")
            elif not rows:
                val = t.detach().to(device="cpu", dtype=torch.float64).tolist()
                if name == "weights":
                    over.update(zip(_WEIGHT_KEYS, val))
                else:
                    over[name] = tuple(val) if shape else val
        given.append(t)
    return over, given, rows


def _param_defaults(p):
    """the solver's own values of the five (p: capi.Params), in _COMPACT_PARAMS' order"""
    return [[getattr(p, k) for k in _WEIGHT_KEYS], p.step_size, p.wheelbase, list(p.lower), list(p.upper)]


def _onto(d, t):
    """a gradient as the given parameter tensor t wants it"""
    return d.to(device=t.device, dtype=t.dtype).reshape(t.shape)


def _scatter_params(g, given, need, per_instance=(False,) * 5):
    """The five parameter gradients out of g["params"] [10] (a per-instance parameter: its own rows of
    g["params_rows"] [10, n]), each onto its given tensor; None where none is needed."""
    return [_onto(g["params_rows" if per else "params"][where], t) if on else None
            for (_, _, where), t, on, per in zip(_COMPACT_PARAMS, given, need, per_instance)]


def compact_general_form(v, delta_y, delta_phi, weights, step_size, wheelbase, lower, upper, horizon, x0=None):
    """The reference controller's model (src/trajectory_point_follower.cpp:326-371) for the speeds v [n] in
    solve_batch_general's form, built with torch ops so that gradients flow: a dict A = [1, Tv; 0, 1],
    B = [0, Tv; Tv/l, -Tv/l], C = 0, Q = (weight_y, weight_phi), R = (weight_steering_front, weight_steering_rear),
    lower, upper, x0 (zeros unless given [2, n]) and targets, (delta_y, delta_phi) at each of `horizon` steps.
    `weights` is [4] or [4, n], `lower` / `upper` [2] or [2, n], T = step_size and l = wheelbase scalars or [n];
    numbers and tensors alike become fp64 tensors on v's device first, never Python divisors, which torch multiplies
    by their reciprocal: the last bit would differ."""
    n = v.shape[-1]
    f64 = dict(dtype=torch.float64, device=v.device)

    def rows(x, k):
        x = torch.as_tensor(x, **f64)
        return (x[:, None] if x.dim() == 1 else x).expand(k, n)

    T = torch.as_tensor(step_size, **f64)
    l = torch.as_tensor(wheelbase, **f64)
    Tv = T * v
    one, zero = torch.ones(n, **f64), torch.zeros(n, **f64)
    w = rows(weights, 4)
    return {"A": torch.stack([one, Tv, zero, one]), "B": torch.stack([zero, Tv, Tv / l, -Tv / l]),
            "C": torch.zeros(2, n, **f64), "Q": w[0:2], "R": w[2:4], "lower": rows(lower, 2), "upper": rows(upper, 2),
            "x0": torch.zeros(2, n, **f64) if x0 is None else x0,
            "targets": torch.stack([delta_y, delta_phi]).repeat(horizon, 1)}


class _MpcGeneral(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, over, polish, A, B, Cc, Q, R, lower, upper, x0, targets):
        I = R.shape[0]
        H = solver._params(**over).horizon
        ins = [t.detach().contiguous() for t in (A, B, Cc, Q, R, lower, upper, x0, targets)]
        controls = torch.zeros((H * I, A.shape[-1]), dtype=torch.float64, device=A.device)
        solver.solve_batch_general(*ins, controls=controls, inputs=I, **over)   # zeros shifted are zeros: a cold start
        if polish:   # onto the verified optimum where it is reached; the others keep the solver's sequence
            tol, rounds = _polish(polish)
            keys = {k: v for k, v in over.items() if k == "horizon"}
            solver.polish_batch_general(*ins, controls, tol=tol, max_rounds=rounds, want_status=False, inputs=I, **keys)
        ctx.solver, ctx.over, ctx.I = solver, over, I
        ctx.save_for_backward(*ins, controls)
        ctx.save_for_forward(*ins, controls)
        return controls

    @staticmethod
    def jvp(ctx, _solver, _over, _polish, *tangents):
        *ins, controls = ctx.saved_tensors
        tan = {k: t.contiguous() for k, t in zip(MODEL_NAMES, tangents) if t is not None}
        if not tan:
            return torch.zeros_like(controls)
        return ctx.solver.solve_batch_general_forward(*ins, controls, tan, inputs=ctx.I, want_flags=False,
                                                      **ctx.over)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_controls):
        *ins, controls = ctx.saved_tensors
        want = tuple(k for k, need in zip(MODEL_NAMES, ctx.needs_input_grad[3:]) if need)
        if not want:
            return (None,) * 12
        g = ctx.solver.solve_batch_general_backward(*ins, controls, grad_controls.contiguous(), inputs=ctx.I,
                                                    want=want, want_flags=False, **ctx.over)
        return (None, None, None) + tuple(g.get(k) for k in MODEL_NAMES)


def mpc_general(solver, A, B, Cc, Q, R, lower, upper, x0, targets, polish=False, **over):
    """The solved control sequence [H*I, n] of n fresh dlib::mpc<2,I,H> controllers (rows 0..I-1 are u0), as a
    differentiable function of the component-major CUDA fp64 tensors A[4,n] B[2I,n] C[2,n] Q[2,n] R[I,n] lower[I,n]
    upper[I,n] x0[2,n] targets[2H,n] (solve_batch_general's layout).  `over` overrides the solver's parameters
    (horizon, eps, max_iter, algo, ...).  polish=True (or a (tol, max_rounds) pair; True is (1e-9, 8)) runs
    MpcSolver.polish_batch_general on the solved sequence before it is returned and saved, so a solve at dlib's eps
    0.01 is differentiated at the optimum; an instance the polish cannot verify keeps the solver's sequence."""
    _require_cuda_f64("mpc_general takes CUDA fp64 tensors", A, B, Cc, Q, R, lower, upper, x0, targets)
    return _MpcGeneral.apply(solver, over, polish, A, B, Cc, Q, R, lower, upper, x0, targets)


class _MpcRollout(torch.autograd.Function):
    """mpc_rollout: the nine arrays, then new_last_targets, Ap, Bp, Cp (all or none) and the disturbance, each of
    which may be None.  A None input needs no gradient and has no tangent, so with no plant and no disturbance no
    plant name reaches the solver and its methods take the entries without a plant."""

    @staticmethod
    def forward(ctx, solver, steps, over, polish, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets, Ap, Bp,
                Cp, disturbance):
        I = R.shape[0]
        ins = [t.detach().contiguous() for t in (A, B, Cc, Q, R, lower, upper, x0, targets)]
        opt = [None if t is None else t.detach().contiguous() for t in (new_last_targets, Ap, Bp, Cp, disturbance)]
        nlt, plant, dist = opt[0], (None if Ap is None else tuple(opt[1:4])), opt[4]
        if polish:   # every step onto the verified optimum before the plant moves; the backward is the same
            tol, rounds, newton_first = polish
            forward = solver.rollout_newton if newton_first else solver.rollout_polished
            controls, states, sequences, *_ = forward(steps, *ins, nlt, inputs=I, tol=tol, max_rounds=rounds,
                                                      want_status=False, plant=plant, disturbance=dist, **over)
        else:
            controls, states, sequences, _ = solver.rollout_record(steps, *ins, nlt, inputs=I, plant=plant,
                                                                   disturbance=dist, **over)
        ctx.solver, ctx.steps, ctx.over, ctx.I = solver, steps, over, I
        ctx.save_for_backward(*ins, *opt, states, sequences)     # (a None is saved as None)
        ctx.save_for_forward(*ins, *opt, states, sequences, controls)
        return controls, states

    @staticmethod
    def _unpack(ctx):
        saved = ctx.saved_tensors
        nlt, Ap, Bp, Cp, dist = saved[9:14]
        return saved[:9], nlt, (None if Ap is None else (Ap, Bp, Cp)), dist, saved[14:]

    @staticmethod
    def jvp(ctx, _solver, _steps, _over, _polish, *tangents):
        ins, nlt, plant, dist, (states, sequences, controls) = _MpcRollout._unpack(ctx)
        tan = {k: t.contiguous() for k, t in zip(_ROLLOUT_NAMES, tangents) if t is not None}
        if not tan:
            return torch.zeros_like(controls), torch.zeros_like(states)
        tu, tx = ctx.solver.rollout_forward(ctx.steps, *ins, nlt, sequences=sequences, states=states, tangents=tan,
                                            inputs=ctx.I, want_flags=False, plant=plant, disturbance=dist, **ctx.over)
        return tu[0], tx[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_controls, grad_states):
        ins, nlt, plant, dist, (states, sequences) = _MpcRollout._unpack(ctx)
        want = tuple(k for k, need in zip(_ROLLOUT_NAMES, ctx.needs_input_grad[4:]) if need)
        if not want:
            return (None,) * 18
        g = ctx.solver.rollout_backward(ctx.steps, *ins, nlt, sequences=sequences, states=states,
                                        grad_controls=_contiguous(grad_controls), grad_states=_contiguous(grad_states),
                                        inputs=ctx.I, want=want, want_flags=False, plant=plant, disturbance=dist,
                                        **ctx.over)
        return (None, None, None, None) + tuple(g.get(k) for k in _ROLLOUT_NAMES)


def mpc_rollout(solver, steps, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets=None, polish=False,
                newton_first=False, plant=None, disturbance=None, **over):
    """The closed loop of n fresh dlib::mpc<2,I,H> controllers (MpcSolver.rollout: `steps` warm-started operator()
    calls with the target shift and the plant update x <- A x + B u + C between them) as a differentiable function.
    Returns (controls [steps*I, n], states [steps*2, n]); gradients reach A, B, C, Q, R, lower, upper, x0, targets and
    new_last_targets [steps*2, n] (component-major CUDA fp64 tensors, solve_batch_general's layout).  Each step is
    differentiated on the active set of its solved sequence (tpc_mpc_rollout_backward, include/tpc_mpc.h); the warm
    start gets no gradient.  That is the derivative of the closed loop when every step's sequence is the optimum, which
    dlib's default eps 0.01 does not give: pass polish=True (or a (tol, max_rounds) pair; True is (1e-9, 8), the
    convention of mpc_general).  The forward is then MpcSolver.rollout_polished -- every step's sequence is moved onto
    the verified optimum before the plant moves, so the loop no longer depends on eps or the warm start beyond tol and
    "no gradient to the warm start" is exact -- and the backward runs on the polished sequences; a step the polish
    cannot verify keeps the solver's sequence.  (A small eps, e.g. eps=1e-10, is the expensive alternative.)
    polish=False is the unpolished loop, bit for bit.  newton_first=True (with polish) makes the forward
    MpcSolver.rollout_newton: every step is polished from the shifted warm start first, all steps in one launch, and
    only the instances it does not verify run rollout_polished's loop; both forwards return the verified optimum of
    every step, so they agree to rounding, and the backward is the same.  `over` overrides the solver's parameters.
    plant=(Ap, Bp, Cp) [4, n] [2I, n] [2, n] and / or disturbance [steps*2, n]: the state moves with
    x <- Ap x + Bp u + Cp + d_k while every step's controller keeps A, B, C (tpc_mpc_rollout_plant); gradients and
    forward_ad tangents then reach Ap, Bp, Cp and the disturbance too, and those of A, B, C are what the controller's
    belief alone contributes.  Both None is the loop on the controller's own model, through the entries without a
    plant."""
    if newton_first and not polish:
        raise ValueError("newton_first needs polish")
    if polish:
        polish = _polish(polish) + (bool(newton_first),)
    _require_cuda_f64("mpc_rollout takes CUDA fp64 tensors", A, B, Cc, Q, R, lower, upper, x0, targets,
                      new_last_targets)
    Ap, Bp, Cp = plant if plant is not None else (None, None, None)
    _require_cuda_f64("mpc_rollout takes CUDA fp64 tensors", Ap, Bp, Cp, disturbance)
    return _MpcRollout.apply(solver, int(steps), over, polish, A, B, Cc, Q, R, lower, upper, x0, targets,
                             new_last_targets, Ap, Bp, Cp, disturbance)


def mpc_compact(solver, v, delta_y, delta_phi, weights, step_size=0.1, wheelbase=0.21,
                lower=(-_ALPHA_MAX, -_ALPHA_MAX), upper=(_ALPHA_MAX, _ALPHA_MAX), polish=False, **over):
    """mpcControllerTobi for n instances as a differentiable function: returns (front, rear), each [n].

    The model is built with torch ops from the reference controller's (src/trajectory_point_follower.cpp:326-371):
    A = [1, Tv; 0, 1], B = [0, Tv; Tv/l, -Tv/l], C = 0, x0 = 0, Q = (weight_y, weight_phi), R = (weight_steering_front,
    weight_steering_rear), one target (delta_y, delta_phi) for every step (compact_general_form) -- and solved by
    mpc_general, so gradients reach v, delta_y, delta_phi, the four weights (a tensor [4] or [4, n]), T, l and the
    bounds by the chain rule.
    The forward runs the general-form kernels, not solve_batch_compact's family: the controls agree with
    solve_batch_compact to the solvers' tolerance, not bit for bit.  polish: as in mpc_general."""
    form = compact_general_form(v, delta_y, delta_phi, weights, step_size, wheelbase, lower, upper,
                                solver._params(**over).horizon)
    u = mpc_general(solver, *form.values(), polish=polish, **over)
    return u[0], u[1]


class _MpcRolloutCompact(torch.autograd.Function):
    """mpc_rollout_compact: forward tpc_mpc_rollout_compact_exact; backward tpc_mpc_rollout_backward on the expansion
    ("expanded") or one call of tpc_mpc_rollout_compact_exact_backward ("fused")"""

    @staticmethod
    def forward(ctx, solver, steps, over, polish, v, delta_y, delta_phi, x0, *params):
        tol, rounds, fused = polish
        ins = [t.detach().contiguous() for t in (v, delta_y, delta_phi)]
        start = None if x0 is None else x0.detach().contiguous()
        ctx.fused = fused
        controls, states, sequences, _, _ = solver.rollout_compact_exact(steps, *ins, start, tol=tol, max_rounds=rounds,
                                                                         want_status=False, **over)
        ctx.solver, ctx.steps, ctx.over = solver, steps, over
        ctx.given = [None if t is None else t.detach() for t in params]
        ctx.save_for_backward(*ins, states, sequences, start)     # (a None is saved as None)
        return controls, states

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_controls, grad_states):
        v, delta_y, delta_phi, states, sequences, x0 = ctx.saved_tensors
        need = ctx.needs_input_grad[4:]      # v, delta_y, delta_phi, x0, then the five parameters
        if not any(need):
            return (None,) * 13
        solver, over = ctx.solver, ctx.over
        grads = dict(sequences=sequences, states=states, grad_controls=_contiguous(grad_controls),
                     grad_states=_contiguous(grad_states), want_flags=False)
        if ctx.fused:
            # one call: only the outputs someone needs; no status, so both routes differentiate the same instances
            want = tuple(k for k, on in zip(_COMPACT_NAMES + ("x0",), need[:4]) if on)
            if any(need[4:]):
                want += ("params",)
            g = solver.rollout_compact_exact_backward(ctx.steps, v, delta_y, delta_phi, x0, want=want, **grads, **over)
            return (None, None, None, None, g.get("v"), g.get("delta_y"), g.get("delta_phi"), g.get("x0"),
                    *_scatter_params(g, ctx.given, need[4:]))
        p = solver._params(**over)
        f64 = dict(dtype=torch.float64, device=v.device)
        with torch.enable_grad():
            # the leaves: the call's own inputs, and the parameters' values as the forward passed them
            leaves = [t.detach().requires_grad_(on) for t, on in zip((v, delta_y, delta_phi), need[:3])]
            leaves.append(None if x0 is None else x0.detach().requires_grad_(need[3]))
            for t, d, on in zip(ctx.given, _param_defaults(p), need[4:]):
                leaves.append(torch.as_tensor(d if t is None else t, **f64).detach().requires_grad_(on))
            lv, ly, lp, lx, *params = leaves
            arr = compact_general_form(lv, ly, lp, *params, horizon=p.horizon, x0=lx)
            want = tuple(k for k, t in arr.items() if t.requires_grad)
            # (the general-form entry reads none of the compact model's ten values, two of which share its arguments' names)
            over = {k: x for k, x in over.items() if k not in _BY_VALUE}
            g = solver.rollout_backward(ctx.steps, *[t.detach().contiguous() for t in arr.values()], None, inputs=2,
                                        want=want, **grads, **over)
            on = [t for t in leaves if t is not None and t.requires_grad]
            got = iter(torch.autograd.grad([arr[k] for k in want], on, [g[k] for k in want], allow_unused=True))
        out = [next(got) if t is not None and t.requires_grad else None for t in leaves]
        out[4:] = [d if d is None else _onto(d, t) for d, t in zip(out[4:], ctx.given)]
        return (None, None, None, None) + tuple(out)


def mpc_rollout_compact(solver, steps, v, delta_y, delta_phi, weights=None, step_size=None, wheelbase=None,
                        lower=None, upper=None, x0=None, polish=(1e-9, 16), backward="expanded", **over):
    """The reference controller's closed loop as a differentiable function: mpcControllerTobi's model rolled forward
    `steps` steps, every step the verified optimum, the target (delta_y, delta_phi) held.  Returns
    (controls [steps*2, n], states [steps*2, n]).  What a tuner wants: weights fitted to one-step steering
    (mpc_compact_exact) say nothing about how the loop behaves; weights fitted through this function do.

    The forward is MpcSolver.rollout_compact_exact (tpc_mpc_rollout_compact_exact: three doubles in per instance, all
    steps in one launch, no general form; the instances the Newton rounds do not verify run the polished loop) with
    polish = (tol, max_rounds).  v, delta_y, delta_phi are CUDA fp64 tensors [n], x0 a CUDA fp64 tensor [2, n] or None
    (zeros).  The shared parameters are tensors `weights` [4] (weight_y, weight_phi, weight_steering_front,
    weight_steering_rear), `step_size` [], `wheelbase` [], `lower` [2] and `upper` [2] on any device, None taking the
    solver's own value (with `over`'s overrides); their values go into tpc_mpc_params by value, as in
    mpc_compact_exact.
    backward="expanded" (the default): tpc_mpc_rollout_backward on the expanded arrays at the recorded sequences and
    states: mpc_compact's torch expansion (compact_general_form: A = [1, Tv; 0, 1], B = [0, Tv; Tv/l, -Tv/l], ...) is
    built in the backward only, and its chain rule carries the gradient to v, delta_y, delta_phi, x0 and every given
    parameter that requires grad; only the expanded arrays that depend on such an input are differentiated.  Its
    gradients equal mpc_rollout's torch graph on the expansion bit for bit.
    backward="fused": one call of tpc_mpc_rollout_compact_exact_backward (MpcSolver.rollout_compact_exact_backward) on
    torch's current stream, which does not materialise the general form either: the reverse sweep over the steps on the
    model built from v, the chain rule folded in the kernel, the shared parameters' gradient summed over the batch on
    the device in a fixed order and sliced onto the given parameter tensors, x0's gradient from dx0; only the outputs
    someone needs are requested.  The same gradients to rounding (the sums over the batch and over the targets are
    taken in another order).  Once-differentiable; no forward mode."""
    if backward not in ("expanded", "fused"):
        raise ValueError(f'backward must be "expanded" or "fused", got {backward!r}')
    _require_cuda_f64("mpc_rollout_compact takes CUDA fp64 tensors v, delta_y, delta_phi and x0", v, delta_y, delta_phi,
                      x0)
    n = v.numel()
    if x0 is not None and tuple(x0.shape) != (2, n):
        raise ValueError(f"x0 must have shape [2, {n}]")
    over, given, _ = _parse_params(over, (weights, step_size, wheelbase, lower, upper))
    tol, rounds = polish
    return _MpcRolloutCompact.apply(solver, int(steps), over, (float(tol), int(rounds), backward == "fused"), v,
                                    delta_y, delta_phi, x0, *given)


class CompactWarmStart:
    """What mpc_compact_exact(..., warm=) carries from one call to the next: the sequence the last forward returned
    ([2H, n], detached), which the next forward hands to the Newton rounds as their start
    (tpc_mpc_solve_batch_compact_exact_from).  One holder per logged batch: the columns are the instances' own optima of
    the previous optimiser step.  The first call, or a call whose n, H or device differs from the stored sequence's,
    is a cold call.  reset() forgets the sequence."""

    def __init__(self):
        self.sequence = None

    def reset(self):
        self.sequence = None

    def start_for(self, H, like):
        s = self.sequence
        if s is None or tuple(s.shape) != (2 * H, like.numel()) or s.device != like.device:
            return None
        return s


def _warm_forward(solver, warm, ins, over, **kw):
    """solve_batch_compact_exact from the holder's sequence (warm None: the cold call), which then takes the returned
    one -- a new tensor every call, so the sequence an earlier forward saved for its backward is never written"""
    start = None if warm is None else warm.start_for(solver._params(**over).horizon, ins[0])
    out = solver.solve_batch_compact_exact(*ins, want_sequence=True, start=start, **kw, **over)
    if warm is not None:
        warm.sequence = out[2].detach()
    return out


def _compact_tangents(tangents):
    return {k: t.contiguous() for k, t in zip(_COMPACT_NAMES, tangents) if t is not None}


class _MpcCompactExact(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, over, polish, v, delta_y, delta_phi, *params):
        tol, rounds, fallback, warm = polish
        ins = [t.detach().contiguous() for t in (v, delta_y, delta_phi)]
        front, rear, sequence, status, _ = _warm_forward(solver, warm, ins, over, tol=tol, max_rounds=rounds,
                                                         fallback=fallback)
        ctx.solver, ctx.over = solver, over
        ctx.given = [None if t is None else t.detach() for t in params]   # where each parameter's gradient goes
        ctx.save_for_backward(*ins, sequence, status)
        ctx.save_for_forward(*ins, sequence, status)
        return front, rear

    @staticmethod
    def jvp(ctx, _solver, _over, _polish, tv, tdy, tdphi, *tparams):
        v, delta_y, delta_phi, sequence, status = ctx.saved_tensors
        tan = _compact_tangents((tv, tdy, tdphi))
        if any(t is not None for t in tparams):
            # the given parameters' tangents, sliced into one row of the ten and moved to v's device
            row = torch.zeros(1, 10, dtype=torch.float64)
            for (_, _, where), t in zip(_COMPACT_PARAMS, tparams):
                if t is not None:
                    row[0, where] = t.detach().to(device="cpu", dtype=torch.float64)
            tan["params"] = row.to(v.device)
        if not tan:
            return torch.zeros_like(v), torch.zeros_like(v)
        tf, tr = ctx.solver.solve_batch_compact_exact_forward(v, delta_y, delta_phi, sequence, tan, status=status,
                                                              want_flags=False, **ctx.over)
        return tf[0], tr[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_front, grad_rear):
        v, delta_y, delta_phi, sequence, status = ctx.saved_tensors
        need = ctx.needs_input_grad[3:]
        want = tuple(k for k, on in zip(_COMPACT_NAMES, need[:3]) if on)
        if any(need[3:]):
            want += ("params",)
        if not want:
            return (None,) * 11
        g = ctx.solver.solve_batch_compact_exact_backward(
            v, delta_y, delta_phi, sequence, grad_front=grad_front.contiguous(), grad_rear=grad_rear.contiguous(),
            status=status, want=want, want_flags=False, **ctx.over)
        return (None, None, None, g.get("v"), g.get("delta_y"), g.get("delta_phi"),
                *_scatter_params(g, ctx.given, need[3:]))


class _MpcCompactExactRows(torch.autograd.Function):
    """mpc_compact_exact with at least one per-instance parameter: the rows entries on a [10, n] device tensor"""

    @staticmethod
    def forward(ctx, solver, over, polish, defaults, v, delta_y, delta_phi, *params):
        tol, rounds, fallback, warm = polish
        ins = [t.detach().contiguous() for t in (v, delta_y, delta_phi)]
        n = ins[0].numel()
        # the ten rows, filled on the device by broadcasting: a given tensor as it is, the solver's value otherwise
        rows = torch.empty(10, n, dtype=torch.float64, device=ins[0].device)
        ctx.per_instance = []
        for (_, _, where), t, default in zip(_COMPACT_PARAMS, params, defaults):
            dst = rows[where]
            if t is None:
                src = torch.tensor(default, dtype=torch.float64).to(rows.device, non_blocking=True)
            else:
                src = t.detach().to(device=rows.device, dtype=torch.float64)
            per = t is not None and t.dim() == dst.dim()
            ctx.per_instance.append(per)
            dst.copy_(src if per else src.unsqueeze(-1))
        front, rear, sequence, status, _ = _warm_forward(solver, warm, ins, over, tol=tol, max_rounds=rounds,
                                                         fallback=fallback, params_rows=rows)
        ctx.solver, ctx.over = solver, over
        ctx.given = [None if t is None else t.detach() for t in params]
        ctx.save_for_backward(*ins, rows, sequence, status)
        ctx.save_for_forward(*ins, rows, sequence, status)
        return front, rear

    @staticmethod
    def jvp(ctx, _solver, _over, _polish, _defaults, tv, tdy, tdphi, *tparams):
        v, delta_y, delta_phi, rows, sequence, status = ctx.saved_tensors
        tan = _compact_tangents((tv, tdy, tdphi))
        if any(t is not None for t in tparams):
            # the ten rows' tangent, by the forward's broadcasting: a shared parameter's next to a per-instance one's
            trows = torch.zeros(1, 10, v.numel(), dtype=torch.float64, device=v.device)
            for (_, _, where), t, per in zip(_COMPACT_PARAMS, tparams, ctx.per_instance):
                if t is not None:
                    src = t.detach().to(device=v.device, dtype=torch.float64)
                    trows[0, where] = src if per else src.unsqueeze(-1)
            tan["params_rows"] = trows
        if not tan:
            return torch.zeros_like(v), torch.zeros_like(v)
        tf, tr = ctx.solver.solve_batch_compact_exact_forward(v, delta_y, delta_phi, sequence, tan, status=status,
                                                              params_rows=rows, want_flags=False, **ctx.over)
        return tf[0], tr[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_front, grad_rear):
        v, delta_y, delta_phi, rows, sequence, status = ctx.saved_tensors
        need = ctx.needs_input_grad[4:]
        want = tuple(k for k, on in zip(_COMPACT_NAMES, need[:3]) if on)
        if any(on and not per for on, per in zip(need[3:], ctx.per_instance)):
            want += ("params",)
        if any(on and per for on, per in zip(need[3:], ctx.per_instance)):
            want += ("params_rows",)
        if not want:
            return (None,) * 12
        g = ctx.solver.solve_batch_compact_exact_backward(
            v, delta_y, delta_phi, sequence, grad_front=grad_front.contiguous(), grad_rear=grad_rear.contiguous(),
            status=status, want=want, want_flags=False, params_rows=rows, **ctx.over)
        # a per-instance parameter: its own rows; a shared one: the batch sum, as it was broadcast to everyone
        return (None, None, None, None, g.get("v"), g.get("delta_y"), g.get("delta_phi"),
                *_scatter_params(g, ctx.given, need[3:], ctx.per_instance))


def mpc_compact_exact(solver, v, delta_y, delta_phi, weights=None, step_size=None, wheelbase=None, lower=None,
                      upper=None, tol=1e-9, max_rounds=16, fallback="solve", warm=None, **over):
    """mpcControllerTobi for n instances, answered with the verified optimum and differentiable: returns
    (front, rear), each [n].  The weights, T, l and bounds are shared by the batch or given per instance.

    The forward is MpcSolver.solve_batch_compact_exact (three doubles in, two out per instance, the sequence and the
    status kept); the backward is one call of tpc_mpc_solve_batch_compact_exact_backward on torch's current stream --
    neither side materialises the general form.  v, delta_y, delta_phi are CUDA fp64 tensors [n].  The shared
    parameters are tensors `weights` [4] (weight_y, weight_phi, weight_steering_front, weight_steering_rear),
    `step_size` [], `wheelbase` [], `lower` [2] and `upper` [2], on any device; None takes the solver's own value
    (with `over`'s overrides).  Their VALUES go into tpc_mpc_params by value: that is one small device-to-host read per
    given parameter and call when they live on the GPU (keep them on the CPU to avoid it).  Gradients reach v,
    delta_y, delta_phi and every given parameter that requires grad (the batch sum, reduced on the device in a fixed
    order, sliced onto the parameter tensors); an instance left unverified (status -1, fallback="none" or a failed
    fallback) or with non-finite data gets zero gradients and adds nothing to the parameters'.  Once-differentiable.
    Forward mode (torch.autograd.forward_ad): one call of tpc_mpc_solve_batch_compact_exact_forward at the saved
    sequence and status, tangents on v, delta_y, delta_phi and every given parameter, shared (one small host-to-device
    copy of the ten tangents per call) or per-instance; the excluded instances' tangents are zero.

    Per-instance parameters: any of them may carry a trailing n -- `weights` [4, n], `step_size` [n], `wheelbase` [n],
    `lower` / `upper` [2, n], CUDA fp64 -- for weights scheduled on speed, logs with different wheelbases or cycle
    times, per-instance steering limits.  The call then goes through the rows entries
    (tpc_mpc_solve_batch_compact_exact_rows and its backward): a [10, n] tensor is filled on the device by broadcasting
    (a shared tensor as it is, None from the solver's parameters; no device-to-host read), a per-instance parameter's
    gradient is its own rows, a shared one's the batch sum.  An instance whose own column is invalid (a negative
    weight, upper < lower, a zero wheelbase) returns (0, 0) and gets zero gradients.  With no per-instance parameter
    the call is exactly the shared one above.

    warm: a CompactWarmStart, kept by the caller across the steps of a fitting loop over the same batch.  The forward
    hands the holder's sequence -- the previous call's optimum, detached -- to the Newton rounds as their start
    (tpc_mpc_solve_batch_compact_exact_from) and then stores the sequence it returns; the first call, or a changed n or
    horizon, is a cold call.  The backward is unchanged: it differentiates at the returned sequence, which is the same
    optimum to rounding.  Shared and per-instance parameters alike.  None is the call above."""
    if warm is not None and not isinstance(warm, CompactWarmStart):
        raise ValueError("warm must be a CompactWarmStart")
    _require_cuda_f64("mpc_compact_exact takes CUDA fp64 tensors v, delta_y, delta_phi", v, delta_y, delta_phi)
    over, given, rows = _parse_params(over, (weights, step_size, wheelbase, lower, upper), v.numel())
    polish = (float(tol), int(max_rounds), fallback, warm)
    if rows:
        return _MpcCompactExactRows.apply(solver, over, polish, _param_defaults(solver._params(**over)), v, delta_y,
                                          delta_phi, *given)
    return _MpcCompactExact.apply(solver, over, polish, v, delta_y, delta_phi, *given)
