"""CHECKER ONLY: the cases of tests/test_presolve_host.py and tests/test_presolve_gpu.py -- inputs, knobs and the sets of
instances AUTO's presolve (csrc/tpc_mpc_api.cpp: presolve_begin / presolve_finish / general_launch) treats differently.

The presolve takes, by PREDICTION, the instances whose lambda (dlib's trace bound of the Hessian, mpc.h:116-123) is at
least (max_iter / 7)^2 to the bit-exact kernels on a side stream; the flag-driven second pass catches the capped
instances it missed and skips what it took.  Per case and instance, from the oracle's iteration counts `oit`:

    taken    lambda >= (max_iter / 7)^2                       what the prediction names
    capped   oit == max_iter                                  what AUTO must return with dlib's bits
    spare    taken & ~capped & (oit > smo_iters)              predicted, converged after all in the projected-gradient
                                                              phase: only a merge can have put dlib's bits there (what
                                                              stops inside the coordinate-descent phase is not queued)

Nothing here knows the kernels: lambda_general restates dlib, solo_limit restates presolve_share.
"""
import numpy as np

GEN_NAMES = ["A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets"]
# the compact model's constants (oracle.bindings: DEFAULT_WEIGHTS, DEFAULT_T, DEFAULT_L)
WEIGHTS, STEP, WHEELBASE = (20.0, 7.0, 0.0005, 10.0), 0.1, 0.21
SMO_ITERS = 50   # dlib's default length of the coordinate-descent phase

MIXED_BINS = {4: 300, 5: 500, 10: 1000, 20: 1000, 30: 1000, 40: 4096}
MIXED_BINS_SWAPPED = {4: 300, 5: 500, 10: 1000, 20: 4096, 30: 1000, 40: 1000}   # the sizes of the N = 20 and N = 40 bins swapped


def lambda_general(A, B, Q, R, H):
    """dlib's trace bound (mpc.h:116-123) per instance, for AoS arrays as synth.general_inputs returns them
    (A[n,4] row-major 2x2, B[n,2I] row-major 2xI, Q[n,2], R[n,I]):
    lam = H sum(R); Tm = diag(Q); H times: lam += trace(B' Tm B); Tm = A' Tm A + diag(Q)."""
    A = np.asarray(A, dtype=np.float64).reshape(-1, 2, 2)
    n = A.shape[0]
    B = np.asarray(B, dtype=np.float64).reshape(n, 2, -1)
    Qd = np.zeros((n, 2, 2))
    Qd[:, 0, 0], Qd[:, 1, 1] = np.asarray(Q, dtype=np.float64).reshape(n, 2).T
    lam = H * np.asarray(R, dtype=np.float64).reshape(n, -1).sum(axis=1)
    Tm = Qd.copy()
    At, Bt = A.transpose(0, 2, 1), B.transpose(0, 2, 1)
    for _ in range(H):
        lam = lam + np.trace(Bt @ Tm @ B, axis1=1, axis2=2)
        Tm = At @ Tm @ A + Qd
    return lam


def compact_model(v, T=STEP, l=WHEELBASE, weights=WEIGHTS):
    """(A, B, Q, R) of the compact form's model, AoS, for lambda_general."""
    v = np.asarray(v, dtype=np.float64)
    n, a, c = len(v), T * v, T * v / l
    A = np.stack([np.ones(n), a, np.zeros(n), np.ones(n)], axis=1)
    B = np.stack([np.zeros(n), a, c, -c], axis=1)
    return A, B, np.tile(weights[:2], (n, 1)), np.tile(weights[2:], (n, 1))


def lambda_compact(v, H):
    return lambda_general(*compact_model(v), H)


def solo_limit(cu_count):
    """The longest queue the presolve's kernel takes: one round of its wavefronts (7 of 16 SIMDs, 8 instances each)."""
    return cu_count * 4 * 7 // 16 * 8


def batch_bound(cu_count):
    """The largest batch a presolve is tried for."""
    return 5 * solo_limit(cu_count)


def threshold(max_iter):
    return (max_iter / 7.0) ** 2


def _compact(n, first=4242):
    def make():
        from trajectory_controller_amd.synth import compact_inputs
        return compact_inputs(40, n, first=first)
    return make


def _general(I):
    def make():
        from trajectory_controller_amd.synth import general_inputs
        return general_inputs(40, 2048, I=I, first=4711)
    return make


def mixed_inputs(bins=MIXED_BINS):
    """(horizons, v, dy, dphi): ONE array of the N = 40 stream, the horizons of `bins` dealt over it in a fixed shuffle."""
    from trajectory_controller_amd.synth import compact_inputs
    hz = np.concatenate([np.full(c, H, dtype=np.int32) for H, c in bins.items()])
    hz = hz[np.random.default_rng(5).permutation(len(hz))]
    return (hz,) + compact_inputs(40, len(hz), first=4242)


# name -> form, inputs (a callable: nothing is generated on import), the knobs that differ from dlib's defaults
CASES = {
    "overflow": dict(form="compact", inputs=_compact(8192), knobs=dict(max_iter=2000)),
    "fits": dict(form="compact", inputs=_compact(4096), knobs=dict(max_iter=2000)),
    "cd_capped": dict(form="compact", inputs=_compact(4096), knobs=dict(max_iter=2000, smo_iters=2000, eps=0.5)),
    "cd_capped_past": dict(form="compact", inputs=_compact(4096), knobs=dict(max_iter=2000, smo_iters=3000, eps=0.01)),
    "general_I1": dict(form="general", I=1, inputs=_general(1), knobs=dict(max_iter=2000)),
    "general_I2": dict(form="general", I=2, inputs=_general(2), knobs=dict(max_iter=2000)),
    "general_I2_default": dict(form="general", I=2, inputs=_general(2), knobs=dict(max_iter=10000)),
    "mixed": dict(form="mixed", inputs=mixed_inputs, knobs=dict(max_iter=2000)),
    "mixed_default": dict(form="mixed", inputs=mixed_inputs, knobs=dict(max_iter=10000)),
}


class Solved:
    """One batch (or one bin of a mixed batch) solved by the oracle: outputs `out` (a tuple of arrays whose first axis is
    the instance), iteration counts and the three sets."""

    def __init__(self, out, oit, lam, knobs):
        self.out, self.oit, self.lam = tuple(out), oit, lam
        self.max_iter = knobs["max_iter"]
        self.smo_iters = knobs.get("smo_iters", SMO_ITERS)
        self.n = len(oit)
        self.taken = lam >= threshold(self.max_iter)
        self.capped = oit == self.max_iter
        self.spare = self.taken & ~self.capped & (oit > self.smo_iters)


def solve_compact(oracle, H, v, dy, dphi, knobs):
    f, r, it = oracle.solve_compact(H, v, dy, dphi, nthreads=8, **knobs)
    return Solved((f, r), it, lambda_compact(v, H), knobs)


def solve_case(oracle, name):
    """The oracle's answer for a case: a Solved, or for a mixed case {horizon: (index array, Solved)}."""
    c = CASES[name]
    x = c["inputs"]()
    if c["form"] == "compact":
        return solve_compact(oracle, 40, *x, c["knobs"])
    if c["form"] == "general":
        u0, _, it = oracle.solve_general(c["I"], 40, *[x[k] for k in GEN_NAMES], nthreads=8, **c["knobs"])
        return Solved((u0,), it, lambda_general(x["A"], x["B"], x["Q"], x["R"], 40), c["knobs"])
    return solve_mixed(oracle, *x, c["knobs"])


def solve_mixed(oracle, hz, v, dy, dphi, knobs):
    out = {}
    for H in sorted(set(hz.tolist())):
        idx = np.flatnonzero(hz == H)
        out[H] = (idx, solve_compact(oracle, H, v[idx], dy[idx], dphi[idx], knobs))
    return out


def check_conditions(name, s, cu_count=256):
    """The conditions a case must meet for the GPU tests not to pass vacuously (asserts; `s` = solve_case's result)."""
    limit = solo_limit(cu_count)
    if name in ("mixed", "mixed_default"):
        s40 = s[40][1]
        assert s40.n <= batch_bound(cu_count) and s40.taken.sum() <= limit, (name, s40.n, int(s40.taken.sum()))
        assert s40.capped.any() and s40.spare.any(), name
        for H, (_, b) in s.items():
            if H == 40:
                continue
            if name == "mixed":
                assert bool(b.capped.any()) == (H in (20, 30)), (name, H, int(b.capped.sum()))
            else:
                assert not b.capped.any(), (name, H, int(b.capped.sum()))
        return
    taken, capped = int(s.taken.sum()), int(s.capped.sum())
    assert s.n <= batch_bound(cu_count), (name, s.n)
    if name == "overflow":
        assert taken > limit, (name, taken, limit)
        assert 0 < capped < s.n and (s.taken & ~s.capped).any(), (name, capped)
        assert s.spare.any(), name
        return
    assert taken <= limit, (name, taken, limit)
    if name == "fits":
        assert s.capped.any() and s.spare.any(), name
    elif name == "cd_capped":
        assert (s.capped & s.taken).any() and (s.capped & ~s.taken).any() and (~s.capped).any(), name
    elif name == "cd_capped_past":
        assert (s.capped & s.taken).any() and (s.capped & ~s.taken).any(), name
    else:
        assert s.capped.any() and s.spare.any() and (~s.taken).any(), name
