"""torch autograd over the batched general-form solve: `mpc_general` and the reference controller's `mpc_compact`,
and over the closed loop: `mpc_rollout` (forward MpcSolver.rollout_record, or rollout_polished with polish=True;
backward tpc_mpc_rollout_backward); and `mpc_compact_exact`, the reference controller with shared or per-instance
parameters on the exact compact solve and its own backward kernel (no general form on either side); and
`mpc_rollout_compact`, the reference controller's closed loop (forward tpc_mpc_rollout_compact_exact, no general form;
backward tpc_mpc_rollout_backward on the expansion, built in the backward only, or with backward="fused" one call of
tpc_mpc_rollout_compact_exact_backward, no general form either; no forward mode).

Forward is MpcSolver.solve_batch_general from a fresh controller (zero controls); backward is
tpc_mpc_solve_batch_general_backward on torch's current stream (include/tpc_mpc.h gives the definition of the
derivative: the active set is read off the returned controls, the free components are differentiated through the
stationarity condition on that set).  The gradient is that of the optimum when the controls are the optimum: dlib's
default eps 0.01 leaves a loose solution, so either pass polish=True (solve at eps 0.01, then a Newton round or two of
tpc_mpc_polish_batch_general onto the verified optimum -- the cheap way) or a small eps (e.g. eps=1e-10).  Inputs are CUDA fp64
tensors; both functions are once-differentiable.  Instances whose data are non-finite or break dlib's requires clause
get zero gradients.

Forward mode (torch.autograd.forward_ad) works on all four functions: the jvp of mpc_general / mpc_compact is
tpc_mpc_solve_batch_general_forward, that of mpc_rollout tpc_mpc_rollout_forward, that of mpc_compact_exact
tpc_mpc_solve_batch_compact_exact_forward (shared or per-instance parameters, no general form), one direction per
dual level, at the same sequences the backward is taken at.  torch.func transforms are not supported.
"""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

_ALPHA_MAX = 22.0 * math.pi / 180.0   # the reference module's steering bounds


class _MpcGeneral(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, over, polish, A, B, Cc, Q, R, lower, upper, x0, targets):
        I = R.shape[0]
        H = solver._params(**over).horizon
        ins = [t.detach().contiguous() for t in (A, B, Cc, Q, R, lower, upper, x0, targets)]
        controls = torch.zeros((H * I, A.shape[-1]), dtype=torch.float64, device=A.device)
        solver.solve_batch_general(*ins, controls=controls, inputs=I, **over)   # zeros shifted are zeros: a cold start
        if polish:   # onto the verified optimum where it is reached; the others keep the solver's sequence
            tol, rounds = (1e-9, 8) if polish is True else polish
            keys = {k: v for k, v in over.items() if k == "horizon"}
            solver.polish_batch_general(*ins, controls, tol=tol, max_rounds=rounds, want_status=False, inputs=I, **keys)
        ctx.solver, ctx.over, ctx.I = solver, over, I
        ctx.save_for_backward(*ins, controls)
        ctx.save_for_forward(*ins, controls)
        return controls

    @staticmethod
    def jvp(ctx, _solver, _over, _polish, *tangents):
        *ins, controls = ctx.saved_tensors
        names = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets")
        tan = {k: t.contiguous() for k, t in zip(names, tangents) if t is not None}
        if not tan:
            return torch.zeros_like(controls)
        return ctx.solver.solve_batch_general_forward(*ins, controls, tan, inputs=ctx.I, want_flags=False,
                                                      **ctx.over)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_controls):
        *ins, controls = ctx.saved_tensors
        names = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets")
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad[3:]) if need)
        if not want:
            return (None,) * 12
        g = ctx.solver.solve_batch_general_backward(*ins, controls, grad_controls.contiguous(), inputs=ctx.I,
                                                    want=want, want_flags=False, **ctx.over)
        return (None, None, None) + tuple(g.get(k) for k in names)


def mpc_general(solver, A, B, Cc, Q, R, lower, upper, x0, targets, polish=False, **over):
    """The solved control sequence [H*I, n] of n fresh dlib::mpc<2,I,H> controllers (rows 0..I-1 are u0), as a
    differentiable function of the component-major CUDA fp64 tensors A[4,n] B[2I,n] C[2,n] Q[2,n] R[I,n] lower[I,n]
    upper[I,n] x0[2,n] targets[2H,n] (solve_batch_general's layout).  `over` overrides the solver's parameters
    (horizon, eps, max_iter, algo, ...).  polish=True (or a (tol, max_rounds) pair; True is (1e-9, 8)) runs
    MpcSolver.polish_batch_general on the solved sequence before it is returned and saved, so a solve at dlib's eps
    0.01 is differentiated at the optimum; an instance the polish cannot verify keeps the solver's sequence."""
    for t in (A, B, Cc, Q, R, lower, upper, x0, targets):
        if not (t.is_cuda and t.dtype == torch.float64):
            raise ValueError("mpc_general takes CUDA fp64 tensors")
    return _MpcGeneral.apply(solver, over, polish, A, B, Cc, Q, R, lower, upper, x0, targets)


class _MpcRollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, steps, over, polish, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets):
        I = R.shape[0]
        ins = [t.detach().contiguous() for t in (A, B, Cc, Q, R, lower, upper, x0, targets)]
        nlt = None if new_last_targets is None else new_last_targets.detach().contiguous()
        if polish:   # every step onto the verified optimum before the plant moves; the backward is the same
            tol, rounds, newton_first = polish
            forward = solver.rollout_newton if newton_first else solver.rollout_polished
            controls, states, sequences, *_ = forward(steps, *ins, nlt, inputs=I, tol=tol, max_rounds=rounds,
                                                      want_status=False, **over)
        else:
            controls, states, sequences, _ = solver.rollout_record(steps, *ins, nlt, inputs=I, **over)
        ctx.solver, ctx.steps, ctx.over, ctx.I = solver, steps, over, I
        ctx.has_nlt = nlt is not None
        ctx.save_for_backward(*ins, *(() if nlt is None else (nlt,)), states, sequences)
        ctx.save_for_forward(*ins, *(() if nlt is None else (nlt,)), states, sequences, controls)
        return controls, states

    @staticmethod
    def jvp(ctx, _solver, _steps, _over, _polish, *tangents):
        saved = list(ctx.saved_tensors)
        ins, rest = saved[:9], saved[9:]
        nlt = rest.pop(0) if ctx.has_nlt else None
        states, sequences, controls = rest
        names = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "new_last_targets")
        tan = {k: t.contiguous() for k, t in zip(names, tangents) if t is not None}
        if not tan:
            return torch.zeros_like(controls), torch.zeros_like(states)
        tu, tx = ctx.solver.rollout_forward(ctx.steps, *ins, nlt, sequences=sequences, states=states, tangents=tan,
                                            inputs=ctx.I, want_flags=False, **ctx.over)
        return tu[0], tx[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_controls, grad_states):
        saved = list(ctx.saved_tensors)
        ins, rest = saved[:9], saved[9:]
        nlt = rest.pop(0) if ctx.has_nlt else None
        states, sequences = rest
        names = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "new_last_targets")
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad[4:]) if need)
        if not want:
            return (None,) * 14
        g = ctx.solver.rollout_backward(ctx.steps, *ins, nlt, sequences=sequences, states=states,
                                        grad_controls=None if grad_controls is None else grad_controls.contiguous(),
                                        grad_states=None if grad_states is None else grad_states.contiguous(),
                                        inputs=ctx.I, want=want, want_flags=False, **ctx.over)
        return (None, None, None, None) + tuple(g.get(k) for k in names)


class _MpcRolloutPlant(torch.autograd.Function):
    """_MpcRollout against a separate plant (tpc_mpc_rollout_plant and its backward / forward): four more inputs, Ap,
    Bp, Cp (all or none) and the disturbance, each of which may be None."""
    NAMES = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets", "new_last_targets", "Ap", "Bp", "Cp",
             "disturbance")

    @staticmethod
    def forward(ctx, solver, steps, over, polish, A, B, Cc, Q, R, lower, upper, x0, targets, new_last_targets, Ap, Bp,
                Cp, disturbance):
        I = R.shape[0]
        ins = [t.detach().contiguous() for t in (A, B, Cc, Q, R, lower, upper, x0, targets)]
        opt = [None if t is None else t.detach().contiguous() for t in (new_last_targets, Ap, Bp, Cp, disturbance)]
        nlt, plant, dist = opt[0], (None if Ap is None else tuple(opt[1:4])), opt[4]
        if polish:
            tol, rounds, newton_first = polish
            forward = solver.rollout_newton if newton_first else solver.rollout_polished
            controls, states, sequences, *_ = forward(steps, *ins, nlt, inputs=I, tol=tol, max_rounds=rounds,
                                                      want_status=False, plant=plant, disturbance=dist, **over)
        else:
            controls, states, sequences, _ = solver.rollout_record(steps, *ins, nlt, inputs=I, plant=plant,
                                                                   disturbance=dist, **over)
        ctx.solver, ctx.steps, ctx.over, ctx.I = solver, steps, over, I
        ctx.given = [t is not None for t in opt]
        kept = [t for t in opt if t is not None]
        ctx.save_for_backward(*ins, *kept, states, sequences)
        ctx.save_for_forward(*ins, *kept, states, sequences, controls)
        return controls, states

    @staticmethod
    def _unpack(ctx):
        saved = list(ctx.saved_tensors)
        ins, rest = saved[:9], saved[9:]
        opt = [rest.pop(0) if g else None for g in ctx.given]
        plant = None if opt[1] is None else tuple(opt[1:4])
        return ins, opt[0], plant, opt[4], rest

    @staticmethod
    def jvp(ctx, _solver, _steps, _over, _polish, *tangents):
        ins, nlt, plant, dist, (states, sequences, controls) = _MpcRolloutPlant._unpack(ctx)
        tan = {k: t.contiguous() for k, t in zip(_MpcRolloutPlant.NAMES, tangents) if t is not None}
        if not tan:
            return torch.zeros_like(controls), torch.zeros_like(states)
        tu, tx = ctx.solver.rollout_forward(ctx.steps, *ins, nlt, sequences=sequences, states=states, tangents=tan,
                                            inputs=ctx.I, want_flags=False, plant=plant, disturbance=dist, **ctx.over)
        return tu[0], tx[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_controls, grad_states):
        ins, nlt, plant, dist, (states, sequences) = _MpcRolloutPlant._unpack(ctx)
        names = _MpcRolloutPlant.NAMES
        want = tuple(k for k, need in zip(names, ctx.needs_input_grad[4:]) if need)
        if not want:
            return (None,) * 18
        g = ctx.solver.rollout_backward(ctx.steps, *ins, nlt, sequences=sequences, states=states,
                                        grad_controls=None if grad_controls is None else grad_controls.contiguous(),
                                        grad_states=None if grad_states is None else grad_states.contiguous(),
                                        inputs=ctx.I, want=want, want_flags=False, plant=plant, disturbance=dist,
                                        **ctx.over)
        return (None, None, None, None) + tuple(g.get(k) for k in names)


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
    belief alone contributes.  Both None is the function above, untouched."""
    if newton_first and not polish:
        raise ValueError("newton_first needs polish")
    if polish:
        polish = ((1e-9, 8) if polish is True else tuple(polish)) + (bool(newton_first),)
    for t in (A, B, Cc, Q, R, lower, upper, x0, targets) + (() if new_last_targets is None else (new_last_targets,)):
        if not (t.is_cuda and t.dtype == torch.float64):
            raise ValueError("mpc_rollout takes CUDA fp64 tensors")
    if plant is not None or disturbance is not None:
        Ap, Bp, Cp = plant if plant is not None else (None, None, None)
        for t in (Ap, Bp, Cp, disturbance):
            if t is not None and not (t.is_cuda and t.dtype == torch.float64):
                raise ValueError("mpc_rollout takes CUDA fp64 tensors")
        return _MpcRolloutPlant.apply(solver, int(steps), over, polish, A, B, Cc, Q, R, lower, upper, x0, targets,
                                      new_last_targets, Ap, Bp, Cp, disturbance)
    return _MpcRollout.apply(solver, int(steps), over, polish, A, B, Cc, Q, R, lower, upper, x0, targets,
                             new_last_targets)


def mpc_compact(solver, v, delta_y, delta_phi, weights, step_size=0.1, wheelbase=0.21,
                lower=(-_ALPHA_MAX, -_ALPHA_MAX), upper=(_ALPHA_MAX, _ALPHA_MAX), polish=False, **over):
    """mpcControllerTobi for n instances as a differentiable function: returns (front, rear), each [n].

    The model is built with torch ops from the reference controller's (src/trajectory_point_follower.cpp:326-371):
    A = [1, Tv; 0, 1], B = [0, Tv; Tv/l, -Tv/l], C = 0, x0 = 0, Q = (weight_y, weight_phi), R = (weight_steering_front,
    weight_steering_rear), one target (delta_y, delta_phi) for every step -- and solved by mpc_general, so gradients
    reach v, delta_y, delta_phi, the four weights (a tensor [4] or [4, n]), T, l and the bounds by the chain rule.
    The forward runs the general-form kernels, not solve_batch_compact's family: the controls agree with
    solve_batch_compact to the solvers' tolerance, not bit for bit.  polish: as in mpc_general."""
    dev, n = v.device, v.shape[-1]
    f64 = dict(dtype=torch.float64, device=dev)
    H = solver._params(**over).horizon

    def rows(x, k):
        x = torch.as_tensor(x, **f64)
        return (x[:, None] if x.dim() == 1 else x).expand(k, n)

    T = torch.as_tensor(step_size, **f64)
    l = torch.as_tensor(wheelbase, **f64)
    Tv = T * v
    one, zero = torch.ones(n, **f64), torch.zeros(n, **f64)
    A = torch.stack([one, Tv, zero, one])
    B = torch.stack([zero, Tv, Tv / l, -Tv / l])
    w = rows(weights, 4)
    targets = torch.stack([delta_y, delta_phi]).repeat(H, 1)
    u = mpc_general(solver, A, B, torch.zeros(2, n, **f64), w[0:2], w[2:4], rows(lower, 2), rows(upper, 2),
                    torch.zeros(2, n, **f64), targets, polish=polish, **over)
    return u[0], u[1]


class _MpcRolloutCompact(torch.autograd.Function):
    """mpc_rollout_compact: forward tpc_mpc_rollout_compact_exact; backward tpc_mpc_rollout_backward on the expansion
    ("expanded") or one call of tpc_mpc_rollout_compact_exact_backward ("fused")"""
    PARAMS = ("weights", "step_size", "wheelbase", "lower", "upper")
    SLICES = {"weights": slice(0, 4), "step_size": 4, "wheelbase": 5, "lower": slice(6, 8), "upper": slice(8, 10)}
    BY_VALUE = ("weight_y", "weight_phi", "weight_steering_front", "weight_steering_rear", "step_size", "wheelbase",
                "lower", "upper")

    @staticmethod
    def forward(ctx, solver, steps, over, polish, v, delta_y, delta_phi, x0, weights, step_size, wheelbase, lower,
                upper):
        tol, rounds, fused = polish
        ins = [t.detach().contiguous() for t in (v, delta_y, delta_phi)]
        start = None if x0 is None else x0.detach().contiguous()
        ctx.fused = fused
        controls, states, sequences, _, _ = solver.rollout_compact_exact(steps, *ins, start, tol=tol, max_rounds=rounds,
                                                                         want_status=False, **over)
        ctx.solver, ctx.steps, ctx.over = solver, steps, over
        ctx.params = [None if t is None else t.detach() for t in (weights, step_size, wheelbase, lower, upper)]
        ctx.has_x0 = start is not None
        ctx.save_for_backward(*ins, states, sequences, *(() if start is None else (start,)))
        return controls, states

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_controls, grad_states):
        v, delta_y, delta_phi, states, sequences, *rest = ctx.saved_tensors
        need = ctx.needs_input_grad[4:]      # v, delta_y, delta_phi, x0, then PARAMS
        if not any(need):
            return (None,) * 13
        solver, over = ctx.solver, ctx.over
        if ctx.fused:
            # one call: only the outputs someone needs; no status, so both routes differentiate the same instances
            want = tuple(k for k, on in zip(("v", "delta_y", "delta_phi", "x0"), need[:4]) if on)
            if any(need[4:]):
                want += ("params",)
            g = solver.rollout_compact_exact_backward(
                ctx.steps, v, delta_y, delta_phi, rest[0] if ctx.has_x0 else None, sequences=sequences, states=states,
                grad_controls=None if grad_controls is None else grad_controls.contiguous(),
                grad_states=None if grad_states is None else grad_states.contiguous(), want=want, want_flags=False,
                **over)
            out = [g.get("v"), g.get("delta_y"), g.get("delta_phi"), g.get("x0")]
            for name, t, on in zip(_MpcRolloutCompact.PARAMS, ctx.params, need[4:]):   # onto the given parameter tensors
                if not on:
                    out.append(None)
                    continue
                d = g["params"][_MpcRolloutCompact.SLICES[name]]
                out.append(d.to(device=t.device, dtype=t.dtype).reshape(t.shape))
            return (None, None, None, None) + tuple(out)
        p = solver._params(**over)
        H, n = p.horizon, v.numel()
        f64 = dict(dtype=torch.float64, device=v.device)
        defaults = ([p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear], p.step_size,
                    p.wheelbase, list(p.lower), list(p.upper))
        with torch.enable_grad():
            # the leaves: the call's own inputs, and the parameters' values as the forward passed them
            leaves = [t.detach().requires_grad_(on) for t, on in zip((v, delta_y, delta_phi), need[:3])]
            leaves.append(rest[0].detach().requires_grad_(need[3]) if ctx.has_x0 else None)
            for t, d, on in zip(ctx.params, defaults, need[4:]):
                leaves.append(torch.as_tensor(d if t is None else t, **f64).detach().requires_grad_(on))
            lv, ly, lp, lx, w, T, l, lo, hi = leaves
            # mpc_compact's expansion, operation for operation
            Tv = T * lv
            one, zero = torch.ones(n, **f64), torch.zeros(n, **f64)
            rows = lambda x: x[:, None].expand(x.shape[0], n)
            arr = {"A": torch.stack([one, Tv, zero, one]), "B": torch.stack([zero, Tv, Tv / l, -Tv / l]),
                   "C": torch.zeros(2, n, **f64), "Q": rows(w[0:2]), "R": rows(w[2:4]), "lower": rows(lo),
                   "upper": rows(hi), "x0": torch.zeros(2, n, **f64) if lx is None else lx,
                   "targets": torch.stack([ly, lp]).repeat(H, 1)}
            want = tuple(k for k, t in arr.items() if t.requires_grad)
            # (the general-form entry reads none of the compact model's ten values, two of which share its arguments' names)
            over = {k: x for k, x in over.items() if k not in _MpcRolloutCompact.BY_VALUE}
            g = solver.rollout_backward(ctx.steps, *[t.detach().contiguous() for t in arr.values()], None,
                                        sequences=sequences, states=states,
                                        grad_controls=None if grad_controls is None else grad_controls.contiguous(),
                                        grad_states=None if grad_states is None else grad_states.contiguous(),
                                        inputs=2, want=want, want_flags=False, **over)
            on = [t for t in leaves if t is not None and t.requires_grad]
            got = iter(torch.autograd.grad([arr[k] for k in want], on, [g[k] for k in want], allow_unused=True))
        out = [next(got) if t is not None and t.requires_grad else None for t in leaves]
        for i, t in enumerate(ctx.params):     # onto the given parameter tensors
            if out[4 + i] is not None:
                out[4 + i] = out[4 + i].to(device=t.device, dtype=t.dtype).reshape(t.shape)
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
    states: mpc_compact's torch expansion (A = [1, Tv; 0, 1], B = [0, Tv; Tv/l, -Tv/l], ...) is built in the backward
    only, and its chain rule carries the gradient to v, delta_y, delta_phi, x0 and every given parameter that requires
    grad; only the expanded arrays that depend on such an input are differentiated.  Its gradients equal mpc_rollout's
    torch graph on the expansion bit for bit.
    backward="fused": one call of tpc_mpc_rollout_compact_exact_backward (MpcSolver.rollout_compact_exact_backward) on
    torch's current stream, which does not materialise the general form either: the reverse sweep over the steps on the
    model built from v, the chain rule folded in the kernel, the shared parameters' gradient summed over the batch on
    the device in a fixed order and sliced onto the given parameter tensors, x0's gradient from dx0; only the outputs
    someone needs are requested.  The same gradients to rounding (the sums over the batch and over the targets are
    taken in another order).  Once-differentiable; no forward mode."""
    if backward not in ("expanded", "fused"):
        raise ValueError(f'backward must be "expanded" or "fused", got {backward!r}')
    for t in (v, delta_y, delta_phi) + (() if x0 is None else (x0,)):
        if not (t.is_cuda and t.dtype == torch.float64):
            raise ValueError("mpc_rollout_compact takes CUDA fp64 tensors v, delta_y, delta_phi and x0")
    n = v.numel()
    if x0 is not None and tuple(x0.shape) != (2, n):
        raise ValueError(f"x0 must have shape [2, {n}]")
    over = dict(over)
    given = []
    for name, t, shape in (("weights", weights, (4,)), ("step_size", step_size, ()), ("wheelbase", wheelbase, ()),
                           ("lower", lower, (2,)), ("upper", upper, (2,))):
        if t is None:
            given.append(None)
            continue
        t = t if torch.is_tensor(t) else torch.as_tensor(t, dtype=torch.float64)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {list(shape)}")
        val = t.detach().to(device="cpu", dtype=torch.float64).tolist()
        if name == "weights":
            over.update(weight_y=val[0], weight_phi=val[1], weight_steering_front=val[2], weight_steering_rear=val[3])
        else:
            over[name] = tuple(val) if shape else val
        given.append(t)
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


class _MpcCompactExact(torch.autograd.Function):
    PARAMS =("weights", "step_size", "wheelbase", "lower", "upper")
    SLICES = {"weights": slice(0, 4), "step_size": 4, "wheelbase": 5, "lower": slice(6, 8), "upper": slice(8, 10)}

    @staticmethod
    def forward(ctx, solver, over, polish, v, delta_y, delta_phi, weights, step_size, wheelbase, lower, upper):
        tol, rounds, fallback, warm = polish
        ins = [t.detach().contiguous() for t in (v, delta_y, delta_phi)]
        front, rear, sequence, status, _ = _warm_forward(solver, warm, ins, over, tol=tol, max_rounds=rounds,
                                                         fallback=fallback)
        ctx.solver, ctx.over = solver, over
        # where each given parameter's gradient goes
        ctx.like = [None if t is None else (t.device, t.dtype, t.shape)
                    for t in (weights, step_size, wheelbase, lower, upper)]
        ctx.save_for_backward(*ins, sequence, status)
        ctx.save_for_forward(*ins, sequence, status)
        return front, rear

    @staticmethod
    def jvp(ctx, _solver, _over, _polish, tv, tdy, tdphi, *tparams):
        v, delta_y, delta_phi, sequence, status = ctx.saved_tensors
        tan = {k: t.contiguous() for k, t in zip(("v", "delta_y", "delta_phi"), (tv, tdy, tdphi)) if t is not None}
        if any(t is not None for t in tparams):
            # the given parameters' tangents, sliced into one row of the ten and moved to v's device
            row = torch.zeros(1, 10, dtype=torch.float64)
            for name, t in zip(_MpcCompactExact.PARAMS, tparams):
                if t is not None:
                    row[0, _MpcCompactExact.SLICES[name]] = t.detach().to(device="cpu", dtype=torch.float64)
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
        want = tuple(k for k, on in zip(("v", "delta_y", "delta_phi"), need[:3]) if on)
        if any(need[3:]):
            want += ("params",)
        if not want:
            return (None,) * 11
        g = ctx.solver.solve_batch_compact_exact_backward(
            v, delta_y, delta_phi, sequence, grad_front=grad_front.contiguous(), grad_rear=grad_rear.contiguous(),
            status=status, want=want, want_flags=False, **ctx.over)
        out = [g.get("v"), g.get("delta_y"), g.get("delta_phi")]
        for name, like, on in zip(_MpcCompactExact.PARAMS, ctx.like, need[3:]):
            if not on:
                out.append(None)
                continue
            d = g["params"][_MpcCompactExact.SLICES[name]]
            out.append(d.to(device=like[0], dtype=like[1]).reshape(like[2]))
        return (None, None, None) + tuple(out)


class _MpcCompactExactRows(torch.autograd.Function):
    """mpc_compact_exact with at least one per-instance parameter: the rows entries on a [10, n] device tensor"""

    @staticmethod
    def forward(ctx, solver, over, polish, defaults, v, delta_y, delta_phi, weights, step_size, wheelbase, lower,
                upper):
        tol, rounds, fallback, warm = polish
        ins = [t.detach().contiguous() for t in (v, delta_y, delta_phi)]
        n = ins[0].numel()
        # the ten rows, filled on the device by broadcasting: a given tensor as it is, the solver's value otherwise
        rows = torch.empty(10, n, dtype=torch.float64, device=ins[0].device)
        ctx.per_instance = []
        for name, t in zip(_MpcCompactExact.PARAMS, (weights, step_size, wheelbase, lower, upper)):
            sl = _MpcCompactExact.SLICES[name]
            dst = rows[sl]
            if t is None:
                src = torch.tensor(defaults[name], dtype=torch.float64).to(rows.device, non_blocking=True)
            else:
                src = t.detach().to(device=rows.device, dtype=torch.float64)
            per = t is not None and t.dim() == dst.dim()
            ctx.per_instance.append(per)
            dst.copy_(src if per else src.unsqueeze(-1))
        front, rear, sequence, status, _ = _warm_forward(solver, warm, ins, over, tol=tol, max_rounds=rounds,
                                                         fallback=fallback, params_rows=rows)
        ctx.solver, ctx.over = solver, over
        ctx.like = [None if t is None else (t.device, t.dtype, t.shape)
                    for t in (weights, step_size, wheelbase, lower, upper)]
        ctx.save_for_backward(*ins, rows, sequence, status)
        ctx.save_for_forward(*ins, rows, sequence, status)
        return front, rear

    @staticmethod
    def jvp(ctx, _solver, _over, _polish, _defaults, tv, tdy, tdphi, *tparams):
        v, delta_y, delta_phi, rows, sequence, status = ctx.saved_tensors
        tan = {k: t.contiguous() for k, t in zip(("v", "delta_y", "delta_phi"), (tv, tdy, tdphi)) if t is not None}
        if any(t is not None for t in tparams):
            # the ten rows' tangent, by the forward's broadcasting: a shared parameter's next to a per-instance one's
            trows = torch.zeros(1, 10, v.numel(), dtype=torch.float64, device=v.device)
            for name, t, per in zip(_MpcCompactExact.PARAMS, tparams, ctx.per_instance):
                if t is not None:
                    src = t.detach().to(device=v.device, dtype=torch.float64)
                    trows[0, _MpcCompactExact.SLICES[name]] = src if per else src.unsqueeze(-1)
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
        want = tuple(k for k, on in zip(("v", "delta_y", "delta_phi"), need[:3]) if on)
        if any(on and not per for on, per in zip(need[3:], ctx.per_instance)):
            want += ("params",)
        if any(on and per for on, per in zip(need[3:], ctx.per_instance)):
            want += ("params_rows",)
        if not want:
            return (None,) * 12
        g = ctx.solver.solve_batch_compact_exact_backward(
            v, delta_y, delta_phi, sequence, grad_front=grad_front.contiguous(), grad_rear=grad_rear.contiguous(),
            status=status, want=want, want_flags=False, params_rows=rows, **ctx.over)
        out = [g.get("v"), g.get("delta_y"), g.get("delta_phi")]
        for name, like, on, per in zip(_MpcCompactExact.PARAMS, ctx.like, need[3:], ctx.per_instance):
            if not on:
                out.append(None)
                continue
            # a per-instance parameter: its own rows; a shared one: the batch sum, as it was broadcast to everyone
            d = g["params_rows" if per else "params"][_MpcCompactExact.SLICES[name]]
            out.append(d.to(device=like[0], dtype=like[1]).reshape(like[2]))
        return (None, None, None, None) + tuple(out)


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
    for t in (v, delta_y, delta_phi):
        if not (t.is_cuda and t.dtype == torch.float64):
            raise ValueError("mpc_compact_exact takes CUDA fp64 tensors v, delta_y, delta_phi")
    specs = (("weights", weights, (4,)), ("step_size", step_size, ()), ("wheelbase", wheelbase, ()),
             ("lower", lower, (2,)), ("upper", upper, (2,)))
    n = v.numel()
    # `weights` [4] at n == 4 is the shared shape: only a tensor one dimension longer than the shared shape is rows
    if any(torch.is_tensor(t) and t.dim() == len(shape) + 1 for _, t, shape in specs):
        given = []
        for name, t, shape in specs:
            if t is not None:
                t = t if torch.is_tensor(t) else torch.as_tensor(t, dtype=torch.float64)
                if tuple(t.shape) == shape + (n,):
                    if not (t.is_cuda and t.dtype == torch.float64):
                        raise ValueError(f"per-instance {name} must be a CUDA fp64 tensor")
                elif tuple(t.shape) != shape:
                    raise ValueError(f"{name} must have shape {list(shape)} or {list(shape + (n,))}")
            given.append(t)
        p = solver._params(**over)
        defaults = {"weights": [p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear],
                    "step_size": p.step_size, "wheelbase": p.wheelbase, "lower": list(p.lower), "upper": list(p.upper)}
        return _MpcCompactExactRows.apply(solver, dict(over), (float(tol), int(max_rounds), fallback, warm), defaults, v,
                                          delta_y, delta_phi, *given)
    over = dict(over)
    given = []
    for name, t, shape in specs:
        if t is None:
            given.append(None)
            continue
        t = t if torch.is_tensor(t) else torch.as_tensor(t, dtype=torch.float64)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {list(shape)}")
        val = t.detach().to(device="cpu", dtype=torch.float64).tolist()
        if name == "weights":
            over.update(weight_y=val[0], weight_phi=val[1], weight_steering_front=val[2],
                        weight_steering_rear=val[3])
        else:
            over[name] = tuple(val) if shape else val
        given.append(t)
    return _MpcCompactExact.apply(solver, over, (float(tol), int(max_rounds), fallback, warm), v, delta_y, delta_phi,
                                  *given)
