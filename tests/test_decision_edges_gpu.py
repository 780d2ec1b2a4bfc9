"""`-m gpu`: dlib's decision edges (dlib_files/dlib/control/mpc.h:289-345) in every solver family, and the any-horizon
kernel (csrc/mpc_generic.hip) at the edges the specialised kernels are tested at.  Cases: tests/model/decision_cases.py;
the conditions that make them worth running are asserted from the oracle alone in tests/test_decision_edges_host.py.

Contracts (the families' own, as everywhere in the suite):
  bit-exact families (LANE, LANEX, the generic kernel; fp32 LANE / generic against the float-typed restatement):
      identical bits of u0, the solved sequence and dlib's v, identical iteration counts;
  tolerance families (WAVE, LANE_FMA / UBG, GROUPG): identical iteration counts and |du| <= 1e-9.
On the twin-input cases the optimum is not unique, so a family that breaks the arg-max tie the other way returns the
mirror image of the oracle's answer -- an O(0.1) difference in >= 70 % of the instances, not a rounding difference.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal, bits_equal32
from tests.model import decision_cases as dc

pytestmark = pytest.mark.gpu

ATOL = 1e-9
ALWAYS, NEVER = 1 << 40, 0
ALGO_LANE_FMA, ALGO_GROUP = 3, 4
GROUP_BUILT = [(10, 2), (10, 4), (20, 2), (20, 4), (20, 8), (40, 4), (40, 8)]   # as tests/test_groupg_gpu.py selects them
SENT = 777.25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _solver(H, algo, dtype="f64", **kw):
    from trajectory_controller_amd import MpcSolver
    return MpcSolver(horizon=H, device=0, dtype=dtype, algo=algo, **kw)


def _family(H, family, dtype="f64", **kw):
    """A handle pinned to one family: 'lane', 'wave', 'lane_fma', 'generic' (any algo at a non-specialised horizon),
    ('wave', group), ('group', G), ('lanex', below)."""
    from trajectory_controller_amd import capi
    name, arg = family if isinstance(family, tuple) else (family, None)
    s = _solver(H, {"generic": "auto", "lanex": "lane"}.get(name, name), dtype=dtype, **kw)
    if name == "wave" and arg is not None:
        s.set_option(capi.OPT_WAVE_GROUP, arg)
    if name == "group":
        s.set_option(capi.OPT_GROUP_LANES, arg)
    if name == "lanex":
        s._check(s._lib.tpc_mpc_x_set_lanex_below(s._h, arg))
    return s


def _exact(family):
    return (family[0] if isinstance(family, tuple) else family) in ("lane", "lanex", "generic")


_cache = {}


def _expected(orc, tag, I, H, g, cin=None, **kw):
    """The oracle's (u0, controls, iters, v) of a case (named by `tag`: the builders are deterministic), computed once
    per module run and left unchanged."""
    key = (orc.dtype, tag, I, H, tuple(sorted(kw.items())))
    if key not in _cache:
        res = orc.solve_general(I, H, *[g[k] for k in dc.GEN_NAMES], controls_in=cin, want_v=True, nthreads=8, **kw)
        for a in res:
            a.setflags(write=False)
        _cache[key] = res
    return _cache[key]


def _solve(s, g, I, H, npdt=np.float64, state="cold", cin=None, expect_algo=None, **over):
    """solve_batch_general on host arrays.  state: 'cold' (u0 and iters only: the fused kernels), 'controls' (controls in
    and out), 'full' (controls and dlib's v in and out).  Returns (u0[n,I], controls[n,H,I] | None, iters, v | None)."""
    n = g["A"].shape[0]
    arrays = [dc.soa(g[k], npdt) for k in dc.GEN_NAMES]
    controls = vstate = None
    if state != "cold":
        controls = np.zeros((H * I, n), dtype=npdt) if cin is None else dc.soa(cin, npdt)
    if state == "full":
        vstate = np.zeros((H * I, n), dtype=npdt)
    if expect_algo is not None:
        s.set_profiling(True)
    u0, it = s.solve_batch_general(*arrays, controls=controls, v_state=vstate, inputs=I, want_iters=True, **over)
    if expect_algo is not None:
        assert s.last_kernel_times()[2] == expect_algo
    return (u0.T, None if controls is None else dc.aos(controls, H, I), it, None if vstate is None else dc.aos(vstate, H, I))


def _check(family, got, want, npdt=np.float64, what=""):
    """got / want: (u0, controls | None, iters, v | None).  The family's contract; on a miss of a tolerance family the
    comparison with the mirror image (the other tie direction) is printed first."""
    eq = bits_equal if npdt == np.float64 else bits_equal32
    gu0, gc, git, gv = got
    wu0, wc, wit, wv = want
    if _exact(family):
        assert np.array_equal(git, wit), (family, what)
        assert eq(gu0, wu0), (family, what)
        if gc is not None:
            assert eq(gc, wc), (family, what)
        if gv is not None:
            assert eq(gv, wv), (family, what)
        return
    pairs = [(gu0, wu0)] + ([(gc, wc)] if gc is not None else []) + ([(gv, wv)] if gv is not None else [])
    err = max(float(np.abs(a - b).max()) for a, b in pairs)
    same = bool(np.array_equal(git, wit))
    if not (same and err <= ATOL):
        ref = gc if gc is not None else gu0
        wref = wc if gc is not None else wu0
        bad = np.abs(ref - wref).reshape(len(ref), -1).max(axis=1) > ATOL
        mir = np.abs(ref - dc.mirror(wref)).reshape(len(ref), -1).max(axis=1) <= ATOL
        print(f"{family} {what}: max |du| {err:.3e}, iteration counts equal {np.mean(git == wit):.4f}, instances off "
              f"{int(bad.sum())}, of which equal to the mirrored oracle answer {int((bad & mir).sum())}")
    assert same, (family, what)
    assert err <= ATOL, (family, what, err)


# ---------------------------------------------------------------------------------------------
# 1. twin-input ties

TWIN_FAMILIES = (
    [("lane", H) for H in (4, 10, 20)] +
    [(("wave", grp), H) for H, grps in ((4, (1, 2, 4)), (10, (1, 2)), (20, (1,))) for grp in grps] +
    [("lane_fma", H) for H in (4, 10, 20)] +
    [(("group", G), H) for H, G in GROUP_BUILT] +
    [(("lanex", below), H) for H in (10, 20, 40) for below in (ALWAYS, NEVER)] +
    [("generic", H) for H in (7, 33)])


def _twin_id(p):
    fam, H = p
    return (fam if isinstance(fam, str) else f"{fam[0]}{'-g' if fam[0] != 'lanex' else ''}"
            f"{fam[1] if fam[0] != 'lanex' else ('-always' if fam[1] else '-never')}") + f"-H{H}"


@pytest.mark.parametrize("cap", dc.TWIN_CAPS)
@pytest.mark.parametrize("fam_h", TWIN_FAMILIES, ids=_twin_id)
def test_twin_ties_fp64(torch_cuda, oracle, fam_h, cap):
    family, H = fam_h
    g = dc.twin_inputs(H)
    want = _expected(oracle, "twin", 2, H, g, max_iter=cap)
    name = family[0] if isinstance(family, tuple) else family
    with _family(H, family, max_iter=cap) as s:
        if name == "lane_fma":      # cold starts only (with the state in or out the request is LANE's)
            _check(family, _solve(s, g, 2, H, expect_algo=ALGO_LANE_FMA), want, what=f"cold cap {cap}")
            return
        if name == "group":
            _check(family, _solve(s, g, 2, H, expect_algo=ALGO_GROUP), want, what=f"cold cap {cap}")
            _check(family, _solve(s, g, 2, H, state="full", expect_algo=ALGO_GROUP), want, what=f"state cap {cap}")
            return
        _check(family, _solve(s, g, 2, H), want, what=f"cold cap {cap}")
        _check(family, _solve(s, g, 2, H, state="controls" if name == "wave" else "full"), want, what=f"state cap {cap}")


@pytest.mark.parametrize("H,group", [(4, 2), (4, 4), (10, 2)])
def test_twin_ties_wave_grouped_kernels(torch_cuda, oracle, H, group):
    """Two / four instances per wavefront are taken only by batches of more than four instances per CU (one wavefront
    per SIMD, mpc_wave_inst.hip), which 512 never is on a whole MI355X: the twin batch repeated until it is."""
    import torch
    g = dc.twin_inputs(H)
    reps = 4 * torch.cuda.get_device_properties(0).multi_processor_count // dc.TWIN_N + 1
    big = {k: np.concatenate([a] * reps) for k, a in g.items()}
    for cap in (3, 10000):
        want = tuple(np.concatenate([a] * reps) for a in _expected(oracle, "twin", 2, H, g, max_iter=cap))
        with _family(H, ("wave", group), max_iter=cap) as s:
            _check(("wave", group), _solve(s, big, 2, H, state="controls"), want, what=f"n {reps * dc.TWIN_N} cap {cap}")


@pytest.mark.parametrize("cap", dc.TWIN_CAPS)
@pytest.mark.parametrize("family,H", [("lane", 4), ("lane", 10), ("lane", 20), ("generic", 7), ("generic", 33)])
def test_twin_ties_fp32(torch_cuda, oracle32, family, H, cap):
    g = {k: a.astype(np.float32) for k, a in dc.twin_inputs(H).items()}
    want = _expected(oracle32, "twin", 2, H, g, max_iter=cap)
    with _family(H, family, dtype="f32", max_iter=cap) as s:
        _check(family, _solve(s, g, 2, H, np.float32), want, np.float32, what=f"cold cap {cap}")
        _check(family, _solve(s, g, 2, H, np.float32, state="full"), want, np.float32, what=f"state cap {cap}")


@pytest.mark.parametrize("family,H", [("generic", 1), ("generic", 64)])
def test_twin_ties_ends_of_the_horizon_range(torch_cuda, oracle, family, H):
    g = dc.twin_inputs(H)
    want = _expected(oracle, "twin", 2, H, g)
    with _family(H, family) as s:
        _check(family, _solve(s, g, 2, H, state="full"), want)


@pytest.mark.parametrize("family,H,dtype", [("lane", 4, "f64"), ("lane", 10, "f64"), ("lane", 20, "f64"), ("lane", 10, "f32"),
                                            (("lanex", ALWAYS), 10, "f64"), (("lanex", ALWAYS), 40, "f64"),
                                            (("lanex", NEVER), 20, "f64"), ("generic", 7, "f64"), ("generic", 33, "f64"),
                                            ("generic", 7, "f32")])
def test_twin_ties_rollout(torch_cuda, oracle, oracle32, family, H, dtype):
    """Six closed-loop steps: the ties persist under the warm-start shift (mpc.h:231-232)."""
    orc, npdt, eq = (oracle, np.float64, bits_equal) if dtype == "f64" else (oracle32, np.float32, bits_equal32)
    n, steps, cap = 48, 6, 500
    g = {k: a.astype(npdt) for k, a in dc.twin_inputs(H, n=n).items()}
    key = ("rollout", dtype, H)
    if key not in _cache:
        _cache[key] = [orc.rollout(2, H, steps, *[g[name][k] for name in dc.GEN_NAMES], max_iter=cap) for k in range(n)]
    wc = np.stack([r[0] for r in _cache[key]])          # [n, steps, 2]
    ws = np.stack([r[1] for r in _cache[key]])
    wit = np.stack([r[2] for r in _cache[key]])
    with _family(H, family, dtype=dtype, max_iter=cap) as s:
        c, st, it = s.rollout(steps, *[dc.soa(g[k], npdt) for k in dc.GEN_NAMES], inputs=2, want_iters=True)
    assert np.array_equal(it.T, wit)
    assert eq(dc.aos(c, steps, 2), wc) and eq(dc.aos(st, steps, 2), ws)


# ---------------------------------------------------------------------------------------------
# 2. zero gradient and the threshold

EDGE_FAMILIES = (
    [("lane", H) for H in (4, 10, 20)] + [(("wave", 1), 4), ("wave", 4), ("wave", 10), ("wave", 20)] +
    [("lane_fma", H) for H in (4, 10, 20)] + [(("group", G), H) for H, G in ((10, 4), (20, 8), (40, 4))] +
    [(("lanex", below), H) for H in (10, 20, 40) for below in (ALWAYS, NEVER)] +
    [("generic", H) for H in (7, 33, 1, 64)])


@pytest.mark.parametrize("fam_h", EDGE_FAMILIES, ids=_twin_id)
def test_threshold_general_form(torch_cuda, oracle, fam_h):
    """|df| == 0, == eps (dlib continues), just below eps, and far above it with a cap of one (only step 0 may move), on
    exactly representable instances where every df[i] is the same value: also an H-way tie across steps."""
    family, H = fam_h
    name = family[0] if isinstance(family, tuple) else family
    state = {"lane_fma": "cold", "wave": "controls"}.get(name, "full")
    below = dc.D_BELOW_EXACT if _exact(family) else dc.D_BELOW_TOL
    cases = [("zero", dc.D_ZERO, {}, {}), ("eps", dc.D_EPS, {}, {}), ("below", below, {}, {}),
             ("cap1", dc.D_ABOVE, dict(bound=dc.TIGHT), dict(max_iter=1))]
    for tag, d, ckw, kw in cases:
        g = dc.threshold_case(H, d, **ckw)
        want = _expected(oracle, ("thr", tag, d), 1, H, g, eps=dc.EPS, **kw)
        with _family(H, family, eps=dc.EPS, **kw) as s:
            got = _solve(s, g, 1, H, state=state)
            flags = s.last_flags
        _check(family, got, want, what=tag)
        seq = got[1] if got[1] is not None else got[0][:, None, :]
        if tag in ("zero", "below"):
            assert np.all(got[2] == 0) and np.all(seq == 0) and flags == 0, (family, tag)
        if tag == "eps":
            assert np.all(got[2] >= 1), (family, tag)
        if tag == "cap1":
            assert np.all(got[2] == 1) and np.all(seq[:, 0, 0] == -dc.TIGHT) and np.all(seq[:, 1:] == 0), (family, tag)


@pytest.mark.parametrize("algo,H", [(a, H) for a in ("lane", "wave", "lane_fma", "group", "auto") for H in (4, 10, 20, 40)
                                    if not (a == "group" and H == 4)] + [("auto", 7), ("auto", 33)])
def test_zero_gradient_compact_form(torch_cuda, algo, H):
    """dy = dphi = 0: every df is exactly 0 in the compact form -- zero iterations, u = 0, no flag, in every family and
    through solve_one."""
    v = np.linspace(0.1, 4.0, 70)
    z = np.zeros(70)
    with _solver(H, algo, eps=dc.EPS) as s:
        f, r, it = s.solve_batch_compact(v, z, z, want_iters=True)
        assert np.all(it == 0) and np.all(f == 0) and np.all(r == 0) and s.last_flags == 0
        if algo in ("lane", "auto"):     # LANE also G lanes per instance (N >= 10), and the one-instance entry
            s._check(s._lib.tpc_mpc_x_set_lanex_below(s._h, ALWAYS))
            f, r, it = s.solve_batch_compact(v, z, z, want_iters=True)
            assert np.all(it == 0) and np.all(f == 0) and np.all(r == 0) and s.last_flags == 0
        if algo == "auto":
            assert s.solve_one(1.5, 0.0, 0.0) == (0.0, 0.0) and s.last_solve_one_flags() == (0, 0)


# ---------------------------------------------------------------------------------------------
# 3. bounds: lo == hi, warm starts exactly on a bound

@pytest.mark.parametrize("I", [1, 2])
@pytest.mark.parametrize("fam_h", [("lane", 10), ("lane", 4), ("wave", 10), (("group", 4), 10), (("group", 8), 20),
                                   (("lanex", ALWAYS), 10), (("lanex", ALWAYS), 40), (("lanex", NEVER), 20),
                                   ("generic", 7), ("generic", 33)], ids=_twin_id)
def test_pinned_inputs_and_starts_on_a_bound(torch_cuda, oracle, fam_h, I):
    family, H = fam_h
    n = 330
    g = dc.pinned_inputs(H, n, I=I)
    cin = dc.on_bound_start(g, H, I, seed=11 + H)
    state = "controls" if family == "wave" else "full"
    with _family(H, family) as s:
        _check(family, _solve(s, g, I, H, state=state), _expected(oracle, "pinned", I, H, g), what="cold")
        want = _expected(oracle, "onbound", I, H, g, cin=cin)
        _check(family, _solve(s, g, I, H, state=state, cin=cin), want, what="on a bound")


# ---------------------------------------------------------------------------------------------
# 4. the generic kernel at the specialised kernels' edges

GENERIC = [(H, dtype) for H in (7, 33) for dtype in ("f64", "f32")]


def _types(oracle, oracle32, dtype):
    return (oracle, np.float64, bits_equal) if dtype == "f64" else (oracle32, np.float32, bits_equal32)


@pytest.mark.parametrize("H,dtype", GENERIC)
def test_generic_phase_boundaries(torch_cuda, oracle, oracle32, H, dtype):
    from trajectory_controller_amd import FLAG_MAX_ITER
    from trajectory_controller_amd.synth import compact_inputs
    orc, npdt, eq = _types(oracle, oracle32, dtype)
    v, dy, dphi = (a.astype(npdt) for a in compact_inputs(H, 320, first=7777))
    for smo, cap in dc.PHASES:
        of, orr, oit = orc.solve_compact(H, v, dy, dphi, max_iter=cap, smo_iters=smo, nthreads=8)
        with _solver(H, "auto", dtype=dtype, smo_iters=smo, max_iter=cap) as s:
            f, r, it = s.solve_batch_compact(v, dy, dphi, want_iters=True)
            flags = s.last_flags
        assert np.array_equal(it, oit), (smo, cap)
        assert eq(f, of) and eq(r, orr), (smo, cap)
        assert bool(flags & FLAG_MAX_ITER) == bool(np.any(oit >= cap)), (smo, cap)


@pytest.mark.parametrize("H,dtype", GENERIC)
def test_generic_zero_qdiag_continue_branch(torch_cuda, oracle, oracle32, H, dtype):
    orc, npdt, eq = _types(oracle, oracle32, dtype)
    g = {k: a.astype(npdt) for k, a in dc.zero_qdiag_inputs(H).items()}
    for smo in (50, 3):
        want = _expected(orc, "qdiag", 1, H, g, smo_iters=smo)
        with _solver(H, "auto", dtype=dtype, smo_iters=smo) as s:
            _check("generic", _solve(s, g, 1, H, npdt, state="full"), want, npdt, what=f"smo {smo}")


@pytest.mark.parametrize("H,dtype", GENERIC)
def test_generic_flagged_instances(torch_cuda, oracle, oracle32, H, dtype):
    """Bad models: not solved (start point, iteration 0, FLAG_BAD_MODEL).  Non-finite inputs of the general form run
    through dlib's arithmetic (a NaN or an Inf in x0: every gradient NaN, iteration 0, the start point) and raise
    FLAG_NONFINITE; in the compact form they are screened (start point, iteration 0).  Neighbours untouched."""
    from trajectory_controller_amd import FLAG_BAD_MODEL, FLAG_NONFINITE
    from trajectory_controller_amd.synth import compact_inputs
    orc, npdt, eq = _types(oracle, oracle32, dtype)
    clean, dirty = dc.flagged_inputs(H)
    clean, dirty = ({k: a.astype(npdt) for k, a in d.items()} for d in (clean, dirty))
    wu0, wc, wit, wv = _expected(orc, "flag-clean", 2, H, clean)
    du0, dcn, dit, dv = _expected(orc, "flag-dirty", 2, H, dirty)
    with _solver(H, "auto", dtype=dtype) as s:
        gu0, gc, git, gv = _solve(s, dirty, 2, H, npdt, state="full")
        assert s.last_flags & FLAG_BAD_MODEL and s.last_flags & FLAG_NONFINITE
        _, _, cit, _ = _solve(s, clean, 2, H, npdt)
        assert s.last_flags & (FLAG_BAD_MODEL | FLAG_NONFINITE) == 0
    bad, nonf = list(dc.BAD_MODELS), list(dc.NONFINITE)
    good = np.ones(len(git), dtype=bool)
    good[bad + nonf] = False
    assert np.all(git[bad] == 0) and np.all(gu0[bad] == 0) and np.all(gc[bad] == 0)
    assert np.all(git[nonf] == 0) and np.all(gc[nonf] == 0)
    assert np.array_equal(git[nonf], dit[nonf]) and eq(gc[nonf], dcn[nonf]) and eq(gu0[nonf], du0[nonf])
    assert np.array_equal(git[good], wit[good]) and np.array_equal(cit, wit)
    assert eq(gu0[good], wu0[good]) and eq(gc[good], wc[good]) and eq(gv[good], wv[good])
    # compact form: screened
    v, dy, dphi = (a.astype(npdt) for a in compact_inputs(H, 130, first=5))
    of, orr, oit = orc.solve_compact(H, v, dy, dphi, nthreads=4)
    v[7], dy[64], dphi[129] = np.nan, np.inf, -np.inf
    with _solver(H, "auto", dtype=dtype) as s:
        f, r, it = s.solve_batch_compact(v, dy, dphi, want_iters=True)
        assert s.last_flags & FLAG_NONFINITE
    scr = [7, 64, 129]
    good = np.ones(130, dtype=bool)
    good[scr] = False
    assert np.all(f[scr] == 0) and np.all(r[scr] == 0) and np.all(it[scr] == 0)
    assert np.array_equal(it[good], oit[good]) and eq(f[good], of[good]) and eq(r[good], orr[good])


@pytest.mark.parametrize("H,dtype", GENERIC)
def test_generic_tiny_batches_and_growing_workspace(torch_cuda, oracle, oracle32, H, dtype):
    """n in {1, 63, 64, 65} (the workspace is strided by n), then 65 -> 600 on one handle (the workspace is reused)."""
    from trajectory_controller_amd.synth import compact_inputs
    orc, npdt, eq = _types(oracle, oracle32, dtype)
    g = {k: a.astype(npdt) for k, a in dc.pinned_inputs(H, 600, I=2, first=4100).items()}
    cin = dc.on_bound_start(g, H, 2, seed=3).astype(npdt)
    vin = np.random.default_rng(4).uniform(-0.3, 0.3, size=cin.shape).astype(npdt)
    wu0, wc, wit, wv = orc.solve_general(2, H, *[g[k] for k in dc.GEN_NAMES], controls_in=cin, v_in=vin, want_v=True, nthreads=8)
    v, dy, dphi = (a.astype(npdt) for a in compact_inputs(H, 600, first=31))
    of, orr, oit = orc.solve_compact(H, v, dy, dphi, nthreads=8)

    def run(s, n):
        controls, vstate = dc.soa(cin[:n], npdt), dc.soa(vin[:n], npdt)
        u0, it = s.solve_batch_general(*[dc.soa(g[k][:n], npdt) for k in dc.GEN_NAMES], controls=controls, v_state=vstate,
                                       inputs=2, want_iters=True)
        assert np.array_equal(it, wit[:n]), n
        assert eq(u0.T, wu0[:n]) and eq(dc.aos(controls, H, 2), wc[:n]) and eq(dc.aos(vstate, H, 2), wv[:n]), n
        f, r, it = s.solve_batch_compact(v[:n], dy[:n], dphi[:n], want_iters=True)
        assert np.array_equal(it, oit[:n]) and eq(f, of[:n]) and eq(r, orr[:n]), n
    for n in (1, 63, 64, 65):
        with _solver(H, "auto", dtype=dtype) as s:
            run(s, n)
    with _solver(H, "auto", dtype=dtype) as s:
        run(s, 65)
        run(s, 600)
        run(s, 65)


@pytest.mark.parametrize("H,dtype", GENERIC)
def test_generic_shard_of_wider_batch(torch_cuda, oracle, oracle32, H, dtype):
    """Columns [37, 107) of 200-wide device arrays (ld = 200, n = 70): the kernel's I/O is strided by ld, its workspace
    by n.  Everything outside the shard's columns is pre-filled and must come back untouched."""
    from trajectory_controller_amd import capi
    from trajectory_controller_amd.synth import general_inputs
    torch = torch_cuda
    orc, npdt, eq = _types(oracle, oracle32, dtype)
    I, n_full, k0, n = 2, 200, 37, 70
    es = np.dtype(npdt).itemsize
    g = {k: a.astype(npdt) for k, a in general_inputs(H, n_full, I=I, first=9).items()}
    rng = np.random.default_rng(8)
    cin = rng.uniform(-0.3, 0.3, size=(n_full, H, I)).astype(npdt)
    vin = rng.uniform(-0.3, 0.3, size=(n_full, H, I)).astype(npdt)
    sl = slice(k0, k0 + n)
    wu0, wc, wit, wv = orc.solve_general(I, H, *[g[k][sl] for k in dc.GEN_NAMES], controls_in=cin[sl], v_in=vin[sl],
                                         want_v=True, nthreads=8)
    arrays = [torch.from_numpy(dc.soa(g[k], npdt)).cuda() for k in dc.GEN_NAMES]
    c_before, v_before = dc.soa(cin, npdt), dc.soa(vin, npdt)
    controls, vstate = torch.from_numpy(c_before).cuda(), torch.from_numpy(v_before).cuda()
    u0 = torch.full((I, n_full), SENT, dtype=controls.dtype, device="cuda:0")
    iters = torch.full((n_full,), -5, dtype=torch.int32, device="cuda:0")
    ptr = lambda t: t.data_ptr() + k0 * es
    io = capi.GeneralIO(inputs=I, n=n, ld=n_full, A=ptr(arrays[0]), B=ptr(arrays[1]), C=ptr(arrays[2]), Q=ptr(arrays[3]),
                        R=ptr(arrays[4]), lower=ptr(arrays[5]), upper=ptr(arrays[6]), x0=ptr(arrays[7]),
                        targets=ptr(arrays[8]), controls_inout=ptr(controls), v_inout=ptr(vstate), u0=ptr(u0),
                        iters=iters.data_ptr() + 4 * k0)
    flags = C.c_uint32(0)
    with _solver(H, "auto", dtype=dtype) as s:
        s._check(s._lib.tpc_mpc_solve_batch_general(s._h, C.byref(s.params), C.byref(io), C.byref(flags), capi.DEVICE, None))
        torch.cuda.synchronize()
    u0, iters, controls, vstate = (t.cpu().numpy() for t in (u0, iters, controls, vstate))
    outside = np.ones(n_full, dtype=bool)
    outside[sl] = False
    assert np.all(u0[:, outside] == SENT) and np.all(iters[outside] == -5)
    assert np.array_equal(controls[:, outside], c_before[:, outside]) and np.array_equal(vstate[:, outside], v_before[:, outside])
    assert np.array_equal(iters[sl], wit)
    assert eq(u0[:, sl].T, wu0) and eq(dc.aos(controls[:, sl], H, I), wc) and eq(dc.aos(vstate[:, sl], H, I), wv)


@pytest.mark.parametrize("H", [7, 1])
def test_generic_rollout_with_new_last_targets(torch_cuda, oracle, H):
    """Eight closed-loop steps with a fresh last target per step; at H = 1 the warm-start and target shifts have nothing
    to shift."""
    from trajectory_controller_amd.synth import general_inputs
    I, n, steps = 2, 65, 8
    g = general_inputs(H, n, I=I, first=3)
    nlt = g["targets"][:, -1:, :] + np.random.default_rng(1).uniform(-0.05, 0.05, size=(n, steps, 2))
    want = [oracle.rollout(I, H, steps, *[g[name][k] for name in dc.GEN_NAMES], new_last_targets=nlt[k]) for k in range(n)]
    with _solver(H, "auto") as s:
        c, st, it = s.rollout(steps, *[dc.soa(g[k]) for k in dc.GEN_NAMES], new_last_targets=dc.soa(nlt), inputs=I,
                              want_iters=True)
    assert np.array_equal(it.T, np.stack([w[2] for w in want]))
    assert bits_equal(dc.aos(c, steps, I), np.stack([w[0] for w in want]))
    assert bits_equal(dc.aos(st, steps, 2), np.stack([w[1] for w in want]))
