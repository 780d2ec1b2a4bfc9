"""Pure-numpy builders for the decision-edge tests (tests/test_decision_edges_host.py, tests/test_decision_edges_gpu.py):
inputs on which dlib's two discrete decisions (dlib_files/dlib/control/mpc.h:289-311) are contested.

* the arg-max: dlib scans i then j ascending with a strict '>', so the LOWEST index wins a tie (twin_inputs,
  threshold_case: exact ties that recur);
* the stop test `max_df < eps`: equality continues (threshold_case puts |df| on, just below and above eps, exactly);
* the bound mask: lo == hi, warm starts exactly on a bound with the gradient pointing either way (pinned_inputs,
  on_bound_start).

Everything is AoS fp64 as trajectory_controller_amd.synth.general_inputs returns it; soa() gives the ABI's layout.
"""
import numpy as np

GEN_NAMES = ["A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets"]
TWIN_N = 512
TWIN_CAPS = (1, 3, 50, 10000)
EPS = 2.0 ** -6


def soa(a, dtype=None):
    """AoS [n, ...] -> component-major [comps, n]; always a fresh array (the library updates controls and v in place, and
    for n = 1 the transpose of a view is already contiguous)."""
    a = np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)
    return np.array(a.reshape(a.shape[0], -1).T, order="C", copy=True)


def aos(a, *shape):
    """component-major [comps, n] -> AoS [n, *shape]."""
    a = np.asarray(a)
    return np.array(a.T, order="C", copy=True).reshape(a.shape[1], *shape)


def twin_inputs(H, n=TWIN_N, first=5):
    """General form, I = 2, input 1 a twin of input 0 (same column of B, same R, same bounds): df[2i] and df[2i+1]
    run the same operations on the same values, so they are bit-equal whenever u[2i] == u[2i+1] -- an exact tie at
    iteration 0 (u = 0) that recurs.  The problem is symmetric under swapping the inputs, so the mirror image of an
    answer (mirror()) is the answer of a solver that breaks every tie the other way."""
    from trajectory_controller_amd.synth import general_inputs
    g = general_inputs(H, n, I=2, first=first)
    B = g["B"].reshape(n, 2, 2)           # B[k, r, j]
    B[:, :, 1] = B[:, :, 0]
    g["B"] = np.ascontiguousarray(B.reshape(n, 4))
    for k in ("R", "lo", "hi"):
        g[k][:, 1] = g[k][:, 0]
    return g


def mirror(controls):
    """The answer with the two inputs swapped (last axis: the input index)."""
    return np.ascontiguousarray(np.asarray(controls)[..., ::-1])


def asymmetric(controls):
    """Per instance: does the answer [n, ..., 2] treat the twin inputs differently?"""
    c = np.asarray(controls)
    return np.any(c[..., 0] != c[..., 1], axis=tuple(range(1, c.ndim - 1))) if c.ndim > 2 else c[:, 0] != c[:, 1]


def threshold_case(H, d, n=70, bound=0.25, R=1.0):
    """General form, I = 1, exactly representable: A = identity, C = 0, x0 = 0, B = (1, 0), Q = (1, 1), targets zero
    except the last step's first component = -d.  With u = 0 the linear term is d at every step (sums with zero and
    products with one only), so every df[i] equals the one value d: an H-way tie across steps, sitting wherever d is put
    against eps.  Bounds +-bound and R dyadic.  n identical instances (more than one wavefront)."""
    one = lambda *v: np.tile(np.array(v, dtype=np.float64), (n, 1))
    tg = np.zeros((n, H, 2))
    tg[:, H - 1, 0] = -d
    return dict(A=one(1.0, 0.0, 0.0, 1.0), B=one(1.0, 0.0), C=one(0.0, 0.0), Q=one(1.0, 1.0), R=one(R),
                lo=one(-bound), hi=one(bound), x0=one(0.0, 0.0), targets=tg)


# d of the four threshold cases (EPS = 2^-6): on zero, on eps, one ulp / 2^-40 relative below it, far above it
D_ZERO = 0.0
D_EPS = EPS
D_BELOW_EXACT = EPS * (1.0 - 2.0 ** -53)      # the largest double below eps: for the bit-exact families
D_BELOW_TOL = EPS * (1.0 - 2.0 ** -40)        # for the tolerance families (WAVE's arg-max tag costs 2^-46 relative)
D_ABOVE = 1.0                                 # with bound 2^-7 the first coordinate step saturates on the bound
TIGHT = 2.0 ** -7


def pinned_inputs(H, n, I=2, first=600):
    """Seeded general-form instances with lo == hi on some inputs (valid for dlib: only hi < lo breaks the requires
    clause): every third instance has input 0 pinned at 0.0625, every fifth has its last input pinned at 0 (where the
    cold start already sits), every seventh at -0.125."""
    from trajectory_controller_amd.synth import general_inputs
    g = general_inputs(H, n, I=I, first=first)
    g["lo"][::3, 0] = g["hi"][::3, 0] = 0.0625
    g["lo"][::5, I - 1] = g["hi"][::5, I - 1] = 0.0
    g["lo"][::7, I - 1] = g["hi"][::7, I - 1] = -0.125
    return g


def on_bound_start(g, H, I, seed):
    """controls_in [n, H, I] with every variable exactly on lo, exactly on hi, or inside, a third each."""
    n = g["A"].shape[0]
    rng = np.random.default_rng(seed)
    where = rng.integers(0, 3, size=(n, H, I))
    inside = rng.uniform(-0.2, 0.2, size=(n, H, I))
    lo, hi = g["lo"][:, None, :], g["hi"][:, None, :]
    return np.ascontiguousarray(np.where(where == 0, lo, np.where(where == 1, hi, inside)))


def shifted(cin):
    """What operator() solves from (mpc.h:231-232): controls[i-1] = controls[i], the last one kept."""
    c = np.array(cin, copy=True)
    c[:, :-1] = cin[:, 1:]
    return c


def gradient_at(g, u):
    """df of mpc.h:275-283 plus the linear term of :258-266 at the controls u [n, H, I], in plain numpy (dense, fp64; not
    bit-exact with dlib: used for the SIGN of the gradient at a start point only)."""
    n, H, I = u.shape
    A = g["A"].reshape(n, 2, 2)
    B = g["B"].reshape(n, 2, I)
    Q, R, C, x0, tg = g["Q"], g["R"], g["C"], g["x0"], g["targets"]
    x = x0
    err = np.empty((n, H, 2))
    for i in range(H):          # the state after i + 1 steps against target[i]
        x = np.einsum("nrc,nc->nr", A, x) + np.einsum("nrj,nj->nr", B, u[:, i]) + C
        err[:, i] = (x - tg[:, i]) * Q
    df = np.empty((n, H, I))
    adj = np.zeros((n, 2))
    for i in range(H - 1, -1, -1):
        adj = err[:, i] + np.einsum("nrc,nr->nc", A, adj)
        df[:, i] = np.einsum("nrj,nr->nj", B, adj) + u[:, i] * R
    return df


def zero_qdiag_inputs(H, n=500):
    """The Q = (2, 0) case of test_zero_qdiag_continue_branch (tests/test_parity_gpu.py) at any horizon: Q_diag[H-1] = 0,
    the `continue` of mpc.h:322."""
    rng = np.random.default_rng(21)
    A = np.tile(np.array([1.0, 1.0, 0.0, 1.0]), (n, 1)) + rng.uniform(-0.05, 0.05, (n, 4)) * np.array([0, 1, 0, 0])
    return dict(A=A, B=np.tile(np.array([0.0, 1.0]), (n, 1)), C=rng.uniform(-0.05, 0.1, (n, 2)),
                Q=np.tile(np.array([2.0, 0.0]), (n, 1)), R=rng.uniform(0.5, 2.0, (n, 1)),
                lo=np.full((n, 1), -0.2), hi=np.full((n, 1), 0.2),
                x0=rng.uniform(-5, 5, (n, 2)) * np.array([1.0, 0.2]), targets=np.zeros((n, H, 2)))


PHASES = ((50, 0), (50, 1), (50, 49), (50, 50), (50, 51), (50, 300), (0, 400), (1, 400), (7, 10000), (200, 10000),
          (1000, 120))     # the (smo_iters, max_iter) list of test_phase_boundaries_vs_oracle
BAD_MODELS = {3: ("R", 0, 0.0), 77: ("Q", 1, -1.0), 200: ("hi", 0, -1.0)}   # R = 0, Q < 0, hi < lo
NONFINITE = {120: ("x0", 0, np.nan), 121: ("x0", 1, np.inf)}


def flagged_inputs(H, n=256, I=2, first=99):
    """test_general_invalid_models_are_flagged's three bad models plus a NaN and an Inf input.  Returns (clean, dirty)."""
    from trajectory_controller_amd.synth import general_inputs
    clean = general_inputs(H, n, I=I, first=first)
    dirty = {k: a.copy() for k, a in clean.items()}
    for k, (name, c, val) in {**BAD_MODELS, **NONFINITE}.items():
        dirty[name][k, c] = val
    return clean, dirty
