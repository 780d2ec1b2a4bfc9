"""tests/model/autograd_parent_common.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

What tests/golden/make_golden_autograd.py and tests/test_autograd_parent_gpu.py share: the cases of
tests/golden/autograd_parent.npz and how one is run.  The recording holds what every public function of
trajectory_controller_amd.autograd returned on the device before the module's Functions, its compact expansion and its
parameter parsing were folded into one copy each: under "H<H>/in/<name>" the inputs of a horizon, under
"H<H>/cot/out<i>_<shape>" and "H<H>/tan/<name>_<shape>" the cotangent of output i and the tangent of an input (drawn
once, when the recording was made, and shared by the cases of a horizon), and under "H<H>/<case>/out<i>",
".../grad_<name>" and ".../jvp<i>" the outputs, the gradient of every differentiable input under the cotangents and the
forward_ad tangent of every output where the function has forward mode.

n = 70 (a full wavefront and a partial one), H = 4 (the compact register kernels) and 7 (the workspace kernels), 3 steps;
the general-form cases have one input at H = 4 and two at H = 7.  The model is mpc_rollout_dense.batch's (mixed active
sets), the compact inputs synth.compact_inputs', the per-instance parameters compact_rows_common.recipe_rows("all"), the
start states compact_loop_common.start_states'.
"""
import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from tests.model import compact_loop_common as cl
from tests.model import compact_rows_common as cr
from tests.model import mpc_grad_dense as dense
from tests.model import mpc_rollout_dense as rd
from tests.model.compact_exact_common import VARIANTS
from trajectory_controller_amd import autograd as ag
from trajectory_controller_amd.synth import compact_inputs

N, STEPS, HORIZONS = 70, 3, (4, 7)
INPUTS = {4: 1, 7: 2}
GENERAL = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets")


class Source:
    """Where a case's drawn arrays come from: made now (gold None: the recording run) or read from the recording.
    `seen` holds every key handed out, i.e. what is an input and not a result."""

    def __init__(self, gold=None, seed=0):
        self.gold, self.seen, self.rng = gold, {}, np.random.default_rng(seed)

    def get(self, key, make):
        if key not in self.seen:
            # (np.array, not ascontiguousarray: a 0-d array stays 0-d)
            self.seen[key] = np.array(make(self.rng), order="C") if self.gold is None else self.gold[key]
        return self.seen[key]


INPUT_NAMES = GENERAL + ("new_last_targets", "Ap", "Bp", "Cp", "disturbance", "v", "delta_y", "delta_phi", "weights_rows",
                         "wheelbase_rows", "start")


def inputs(H, src):
    """every array the cases of horizon H read, by name (INPUT_NAMES)"""
    made = _make_inputs(H) if src.gold is None else dict.fromkeys(INPUT_NAMES)
    return {k: src.get(f"H{H}/in/{k}", lambda _, a=a: a) for k, a in made.items()}


def _make_inputs(H):
    I, n, S = INPUTS[H], N, STEPS
    th, nlt = rd.batch(I, H, S, n, seed=H + I, with_nlt=True)
    made = dict(zip(GENERAL, (dense.soa(th[k], n) for k in rd.NAMES)))
    made["new_last_targets"] = dense.soa(nlt, n)
    made["Ap"], made["Bp"], made["Cp"] = made["A"].copy(), made["B"].copy(), made["C"].copy()
    made["Ap"][1] *= 1.05      # a copy of the model with one perturbed row
    made["disturbance"] = 0.002 * np.random.default_rng(70 + H).standard_normal((2 * S, n))
    made["v"], made["delta_y"], made["delta_phi"] = compact_inputs(H, n)
    rows = cr.recipe_rows("all", H, n)
    made["weights_rows"], made["wheelbase_rows"] = rows[cr.W], rows[cr.L]
    made["start"] = cl.start_states(H, n)
    assert tuple(made) == INPUT_NAMES
    return made


def record(prefix, shared, src, fn, leaves, forward=True):
    """fn(**leaves) -> outputs: the outputs, the gradients of every leaf under drawn cotangents, and (forward) the
    forward_ad tangents of the outputs under drawn tangents of every leaf; the draws go by name and shape under
    `shared`, so the cases of a horizon share them"""
    out = {}
    shape = lambda t: "x".join(str(d) for d in t.shape)
    req = {k: t.detach().clone().requires_grad_(True) for k, t in leaves.items()}
    outs = fn(**req)
    cots = []
    for i, o in enumerate(outs):
        out[f"out{i}"] = o
        c = src.get(f"{shared}/cot/out{i}_{shape(o)}", lambda rng, o=o: rng.standard_normal(tuple(o.shape)))
        cots.append(torch.from_numpy(c).to(o.device))
    grads = torch.autograd.grad(outs, list(req.values()), cots, allow_unused=True)
    out.update({f"grad_{k}": g for k, g in zip(req, grads) if g is not None})
    if forward:
        with fwAD.dual_level():
            duals = {}
            for k, t in leaves.items():
                d = src.get(f"{shared}/tan/{k}_{shape(t)}", lambda rng, t=t: rng.standard_normal(tuple(t.shape)))
                duals[k] = fwAD.make_dual(t.detach().clone(), torch.from_numpy(d).to(device=t.device, dtype=t.dtype))
            for i, o in enumerate(fn(**duals)):
                tangent = fwAD.unpack_dual(o).tangent
                if tangent is not None:
                    out[f"jvp{i}"] = tangent
    return {f"{prefix}/{k}": t.detach().cpu().numpy() for k, t in out.items()}


def _cases(H):
    """{case: (fn(solver, **leaves) -> outputs, names of its leaves among `inputs` (or name -> tensor maker), forward)}"""
    S = STEPS
    cpu = lambda x, dtype=torch.float64: (lambda: torch.tensor(x, dtype=dtype))
    w = VARIANTS["weights"]
    weights = [w["weight_y"], w["weight_phi"], w["weight_steering_front"], w["weight_steering_rear"]]
    compact = ("v", "delta_y", "delta_phi")

    def general(**kw):
        return lambda s, **t: (ag.mpc_general(s, *[t[k] for k in GENERAL], **kw),)

    def rollout(nlt=False, plant=False, dist=False, **kw):
        def fn(s, **t):
            return ag.mpc_rollout(s, S, *[t[k] for k in GENERAL], t.get("new_last_targets"),
                                  plant=(t["Ap"], t["Bp"], t["Cp"]) if plant else None,
                                  disturbance=t.get("disturbance"), **kw)
        names = GENERAL + (("new_last_targets",) if nlt else ()) + (("Ap", "Bp", "Cp") if plant else ()) \
            + (("disturbance",) if dist else ())
        return fn, names, True

    def warm_twice(s, **t):
        warm = ag.CompactWarmStart()
        return ag.mpc_compact_exact(s, **t, warm=warm) + ag.mpc_compact_exact(s, **t, warm=warm)

    def loop(backward, x0):
        def fn(s, **t):
            t = dict(t)
            return ag.mpc_rollout_compact(s, S, t.pop("v"), t.pop("delta_y"), t.pop("delta_phi"),
                                          x0=t.pop("start", None), backward=backward, **t)
        leaves = {k: k for k in compact + (("start",) if x0 else ())}
        leaves.update(weights=cpu(weights), step_size=cpu(w["step_size"]))
        return fn, leaves, False

    on_device = {"weights": lambda: torch.tensor(weights, dtype=torch.float64, device="cuda"),
                 "step_size": lambda: torch.tensor(0.08, dtype=torch.float64, device="cuda"),
                 "wheelbase": lambda: torch.tensor(0.25, dtype=torch.float64, device="cuda"),
                 "lower": lambda: torch.tensor([-0.3, -0.2], dtype=torch.float64, device="cuda"),
                 "upper": lambda: torch.tensor([0.25, 0.35], dtype=torch.float64, device="cuda")}
    cases = {
        "general": (general(), GENERAL, True),
        "general_polish": (general(polish=True), GENERAL, True),
        "compact": (lambda s, **t: ag.mpc_compact(s, **t), {**{k: k for k in compact}, **on_device}, True),
        "rollout": rollout(),
        "rollout_nlt": rollout(nlt=True),
        "rollout_polish": rollout(nlt=True, polish=True),
        "rollout_newton": rollout(nlt=True, polish=True, newton_first=True),
        "rollout_plant": rollout(nlt=True, plant=True),
        "rollout_disturbance": rollout(dist=True),
        "exact": (lambda s, **t: ag.mpc_compact_exact(s, **t), compact, True),
        # (a float32 parameter: its gradient and tangent come back as float32)
        "exact_given": (lambda s, **t: ag.mpc_compact_exact(s, **t),
                        {**{k: k for k in compact}, "weights": cpu(weights),
                         "wheelbase": cpu(w["wheelbase"], torch.float32)}, True),
        "exact_rows": (lambda s, **t: ag.mpc_compact_exact(s, **t),
                       {**{k: k for k in compact}, "weights": "weights_rows", "wheelbase": "wheelbase_rows"}, True),
        "exact_warm": (warm_twice, compact, True),
    }
    for backward in ("expanded", "fused"):
        for x0 in (False, True):
            cases[f"loop_{backward}" + ("_x0" if x0 else "")] = loop(backward, x0)
    return cases


def case_names():
    return list(_cases(HORIZONS[0]))


def run_case(H, case, solver, src):
    """the results of one case, {key of the recording: numpy array}; src.seen then also holds what it drew"""
    ins = inputs(H, src)
    fn, leaves, forward = _cases(H)[case]
    leaves = leaves if isinstance(leaves, dict) else {k: k for k in leaves}
    tensors = {k: torch.from_numpy(ins[a]).cuda() if isinstance(a, str) else a() for k, a in leaves.items()}
    return record(f"H{H}/{case}", f"H{H}", src, lambda **t: fn(solver, **t), tensors, forward)
