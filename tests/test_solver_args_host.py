"""CPU tests of MpcSolver's argument rules on a host-only handle (MpcSolver(device=None)), H = 4, I = 2, n = 8, 2 steps.

The rule every array-taking method follows (trajectory_controller_amd/_arrays.py): an array the library only reads is
coerced on the numpy side -- a non-contiguous view, float32 or nested lists give the bits of the contiguous fp64 call --
an array it writes into (controls, v_state, residuals) must already be a C-contiguous fp64 ndarray of the shape, a wrong
row count anywhere is a ValueError before the C call, and None goes through for every optional array.

The coercion is checked for the entries a host-only handle serves; the shape and strictness checks run before the C
call, so the same handle is enough for the entries that need the device.  Every base array is rounded through float32
first, so that its float32 variant holds the same values.  What the tables leave out, because the code before the
helper did otherwise: the numpy plant= / disturbance= of rollout_record / rollout_polished / rollout_newton had to be
contiguous fp64 already (they are coerced now, like rollout_backward's always were), tangents have to be arrays, not
lists (their ndim gives K), and the lengths of delta_y / delta_phi of the compact forward entries went to C unchecked
(test_compact_vector_lengths_are_checked)."""
import functools

import numpy as np
import pytest

from trajectory_controller_amd import MpcSolver, capi
from trajectory_controller_amd.synth import compact_inputs, general_inputs

H, I, N, S, K = 4, 2, 8, 2, 2
MODEL = ("A", "B", "C", "Q", "R", "lower", "upper", "x0", "targets")
PLANT = ("Ap", "Bp", "Cp")
NP = len(capi.COMPACT_PARAM_NAMES)


def f32_exact(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def base():
    """Every argument of every entry, contiguous, float32-representable: computed once, never written."""
    g = general_inputs(H, N, I=I)
    rng = np.random.default_rng(7)
    a = {k: f32_exact(g[s].reshape(N, -1).T) for k, s in zip(MODEL, ("A", "B", "C", "Q", "R", "lo", "hi", "x0", "targets"))}
    a["nlt"] = f32_exact(np.tile(a["targets"][-2:], (S, 1)) + 0.05 * rng.standard_normal((2 * S, N)))
    for k, src in zip(PLANT, ("A", "B", "C")):
        a[k] = f32_exact(a[src] * (1.0 + 0.05 * rng.standard_normal(a[src].shape)))
    a["disturbance"] = f32_exact(0.005 * rng.standard_normal((2 * S, N)))
    a["controls"], a["v_state"] = np.zeros((H * I, N)), np.zeros((H * I, N))
    a["rin"], a["rout"] = np.zeros((S, N)), np.zeros((S, N))
    with MpcSolver(horizon=H, device=None) as s:
        c = s.polish_batch_general(*[a[k] for k in MODEL], np.zeros((H * I, N)), inputs=I, want_status=False)
        _, x, q, _, _, _ = s.rollout_newton(S, *[a[k] for k in MODEL], a["nlt"], inputs=I, fallback="none")
    a["solved"], a["sequences"], a["states"] = f32_exact(c), f32_exact(q), f32_exact(x)
    a["grad_solved"] = f32_exact(rng.standard_normal((H * I, N)))
    a["grad_controls"], a["grad_states"] = f32_exact(rng.standard_normal((S * I, N))), f32_exact(rng.standard_normal((2 * S, N)))
    rows = dict(zip(MODEL, (4, 2 * I, 2, 2, I, I, I, 2, 2 * H)), nlt=2 * S, Ap=4, Bp=2 * I, Cp=2, disturbance=2 * S)
    for k, r in rows.items():
        a["t:" + k] = f32_exact(rng.standard_normal((K, r, N)))
    v, dy, dphi = compact_inputs(H, N)
    a["v"], a["dy"], a["dphi"] = f32_exact(v), f32_exact(dy), f32_exact(dphi)
    p = capi.default_params(H)
    shared = [p.weight_y, p.weight_phi, p.weight_steering_front, p.weight_steering_rear, p.step_size, p.wheelbase,
              p.lower[0], p.lower[1], p.upper[0], p.upper[1]]
    a["params_rows"] = f32_exact(np.array(shared)[:, None] * (1.0 + 0.05 * rng.random((NP, N))))
    a["start"] = f32_exact(0.05 * rng.standard_normal((2 * H, N)))
    a["sequence"] = f32_exact(0.1 * rng.standard_normal((2 * H, N)))
    a["grad_front"], a["grad_rear"] = f32_exact(rng.standard_normal(N)), f32_exact(rng.standard_normal(N))
    a["grad_sequence"] = f32_exact(rng.standard_normal((2 * H, N)))
    a["status"] = np.array([1, 2, -1, 3, 0, 1, -1, 2], dtype=np.int32)
    a["horizons"] = np.full(N, H, dtype=np.int32)
    for x in a.values():
        x.flags.writeable = False
    return a


def model(a):
    return [a[k] for k in MODEL]


def opt(a, *keys):
    return {k: a[k] for k in keys if k in a}


def tangents(a):
    return {("new_last_targets" if k == "t:nlt" else k[2:]): x for k, x in a.items() if k.startswith("t:")}


def plant(a):
    return dict(plant=tuple(a[k] for k in PLANT) if "Ap" in a else None, disturbance=a.get("disturbance"))


def residuals(a):
    if "rin" not in a and "rout" not in a:
        return dict(residuals=None)
    return dict(residuals=(a.get("rin", np.zeros((S, N))), a.get("rout", np.zeros((S, N)))))


# name -> (call(solver, args) -> outputs, the arrays it reads, the arrays it writes into, served by a host-only handle);
# the call's base arguments are the reads plus what HOST_BASE adds; a written array is passed only where a test asks
ENTRIES = {
    "solve_batch_general": (
        lambda s, a: s.solve_batch_general(*model(a), inputs=I, **opt(a, "controls", "v_state")),
        MODEL, ("controls", "v_state"), False),
    "polish_batch_general": (
        lambda s, a: s.polish_batch_general(*model(a), a["controls"], inputs=I),
        MODEL, ("controls",), True),
    "solve_batch_general_backward": (
        lambda s, a: s.solve_batch_general_backward(*model(a), a["solved"], a["grad_solved"], inputs=I),
        MODEL + ("solved", "grad_solved"), (), True),
    "solve_batch_general_forward": (
        lambda s, a: s.solve_batch_general_forward(*model(a), a["solved"], tangents(a), inputs=I),
        MODEL + ("solved",) + tuple("t:" + k for k in MODEL), (), True),
    "rollout": (
        lambda s, a: s.rollout(S, *model(a), a.get("nlt"), inputs=I, **opt(a, "controls", "v_state")),
        MODEL + ("nlt",), ("controls", "v_state"), False),
    "rollout_record": (
        lambda s, a: s.rollout_record(S, *model(a), a.get("nlt"), inputs=I, **opt(a, "controls", "v_state"), **plant(a)),
        MODEL + ("nlt",) + PLANT + ("disturbance",), ("controls", "v_state"), False),
    "rollout_polished": (
        lambda s, a: s.rollout_polished(S, *model(a), a.get("nlt"), inputs=I, **opt(a, "controls", "v_state"),
                                        **residuals(a), **plant(a)),
        MODEL + ("nlt",) + PLANT + ("disturbance",), ("controls", "v_state", "rin", "rout"), False),
    "rollout_newton": (
        lambda s, a: s.rollout_newton(S, *model(a), a.get("nlt"), inputs=I, fallback="none", want_iters=True,
                                      **opt(a, "controls", "v_state"), **residuals(a), **plant(a)),
        MODEL + ("nlt",), ("controls", "v_state", "rin", "rout"), True),
    "rollout_newton[plant]": (
        lambda s, a: s.rollout_newton(S, *model(a), a.get("nlt"), inputs=I, fallback="none", **plant(a)),
        PLANT + ("disturbance",), (), None),          # the shape checks of the plant's arrays only (see the docstring)
    "rollout_backward": (
        lambda s, a: s.rollout_backward(S, *model(a), a.get("nlt"), sequences=a["sequences"], states=a["states"],
                                        inputs=I, **opt(a, "grad_controls", "grad_states"), **plant(a)),
        MODEL + ("nlt", "sequences", "states", "grad_controls", "grad_states") + PLANT, (), True),
    "rollout_forward": (
        lambda s, a: s.rollout_forward(S, *model(a), a.get("nlt"), sequences=a["sequences"], states=a["states"],
                                       tangents=tangents(a), inputs=I, **plant(a)),
        MODEL + ("nlt", "sequences", "states") + PLANT + tuple("t:" + k for k in MODEL + ("nlt",) + PLANT + ("disturbance",)),
        (), True),
    "solve_batch_compact_exact": (
        lambda s, a: s.solve_batch_compact_exact(a["v"], a["dy"], a["dphi"], fallback="none", want_sequence=True,
                                                 want_residuals=True, **opt(a, "params_rows", "start")),
        ("v", "dy", "dphi", "params_rows", "start"), (), True),
    "solve_batch_compact_exact_backward": (
        lambda s, a: s.solve_batch_compact_exact_backward(
            a["v"], a["dy"], a["dphi"], a["sequence"], want=MpcSolver.COMPACT_GRAD_NAMES,
            **opt(a, "grad_front", "grad_rear", "grad_sequence", "status", "params_rows")),
        ("v", "dy", "dphi", "sequence", "grad_front", "grad_rear", "grad_sequence", "status", "params_rows"), (), True),
}
HOST_BASE = {"polish_batch_general": ("controls",)}
# required by the signature: everything else of an entry's arrays may be None
REQUIRED = set(MODEL) | {"solved", "grad_solved", "sequences", "states", "v", "dy", "dphi", "sequence"}
HOST_SERVED = [k for k, e in ENTRIES.items() if e[3]]
READS = [(k, r) for k in HOST_SERVED for r in ENTRIES[k][1]]
CHECKED = [(k, r) for k, e in ENTRIES.items() for r in e[1] + e[2]
           # the compact forward entry reads its three vectors by length alone (below)
           if not (k == "solve_batch_compact_exact" and r in ("v", "dy", "dphi"))]
WRITTEN = [(k, w) for k, e in ENTRIES.items() for w in e[2]]


def arguments(name, **replace):
    """The entry's base call: its read arrays (and a fresh copy of what the base call writes into)"""
    _, reads, _, _ = ENTRIES[name]
    a = {k: base()[k] for k in reads}
    if name.endswith("[plant]"):
        a.update({k: base()[k] for k in MODEL + ("nlt",)})
    a.update({k: base()[k].copy() for k in HOST_BASE.get(name, ())})
    a.update(replace)
    return a


def outputs(res):
    res = list(res.values()) if isinstance(res, dict) else list(res) if isinstance(res, tuple) else [res]
    return [np.asarray(x) for x in res if x is not None]


@functools.lru_cache(maxsize=None)
def contiguous_call(name):
    with MpcSolver(horizon=H, device=None) as s:
        return outputs(ENTRIES[name][0](s, arguments(name)))


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        return bool(np.all(np.ascontiguousarray(a).view(np.uint64) == np.ascontiguousarray(b).view(np.uint64)))
    return np.array_equal(a, b)


def variants(key, x):
    """(label, the same values another way) for a read array"""
    if x.ndim == 1:
        view = np.repeat(x, 2)[::2]
    else:
        view = np.ascontiguousarray(np.swapaxes(x, -1, -2)).swapaxes(-1, -2)   # transposed, then transposed back
    assert not view.flags.c_contiguous and np.array_equal(view, x)
    out = [("view", view)]
    if x.dtype == np.float64:
        out.append(("float32", x.astype(np.float32)))
    else:
        out.append(("int64", x.astype(np.int64)))
    if not key.startswith("t:"):
        out.append(("lists", x.tolist()))
    return out


@pytest.mark.parametrize("name,key", READS, ids=[f"{k}-{r}" for k, r in READS])
def test_read_arrays_are_coerced_to_the_bits_of_the_contiguous_call(name, key):
    want = contiguous_call(name)
    assert want and all(np.all(np.isfinite(x)) for x in want)
    with MpcSolver(horizon=H, device=None) as s:
        for label, x in variants(key, base()[key]):
            got = outputs(ENTRIES[name][0](s, arguments(name, **{key: x})))
            assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want)), (name, key, label)


def one_more_row(x):
    shape = list(x.shape)
    shape[-2 if x.ndim > 1 else 0] += 1
    return np.zeros(shape, dtype=x.dtype)


@pytest.mark.parametrize("name,key", CHECKED, ids=[f"{k}-{r}" for k, r in CHECKED])
def test_a_wrong_row_count_is_a_value_error(name, key):
    with MpcSolver(horizon=H, device=None) as s:
        with pytest.raises(ValueError):
            ENTRIES[name][0](s, arguments(name, **{key: one_more_row(base()[key])}))


@pytest.mark.parametrize("name,key", WRITTEN, ids=[f"{k}-{w}" for k, w in WRITTEN])
def test_written_arrays_are_never_coerced(name, key):
    x = base()[key]
    other = {"rin": "rout", "rout": "rin"}.get(key)
    extra = {other: base()[other].copy()} if other else {}
    with MpcSolver(horizon=H, device=None) as s:
        for bad in (x.astype(np.float32), np.ascontiguousarray(x.T).T, x.tolist()):
            with pytest.raises(ValueError):
                ENTRIES[name][0](s, arguments(name, **{key: bad}, **extra))


@pytest.mark.parametrize("name", [k for k in ENTRIES if not k.endswith("[plant]")])
def test_none_goes_through_for_every_optional_array(name):
    _, reads, writes, _ = ENTRIES[name]
    optional = [k for k in reads + writes if k not in REQUIRED and not k.startswith("t:")
                and not (name == "polish_batch_general" and k == "controls")]
    a = {k: v for k, v in arguments(name).items() if k not in optional}
    if any(k.startswith("t:") for k in reads):      # a missing tangent is a zero tangent; one has to be there
        a = {k: v for k, v in a.items() if not k.startswith("t:") or k == "t:x0"}
    with MpcSolver(horizon=H, device=None) as s:
        try:
            res = outputs(ENTRIES[name][0](s, a))
        except capi.TpcMpcError as e:               # the library's own answer: this handle has no device
            assert not ENTRIES[name][3] and e.status == 6, e
        else:
            assert ENTRIES[name][3] and res


def test_mixed_horizons_and_compact_shapes():
    a = base()
    with MpcSolver(horizon=H, device=None) as s:
        with pytest.raises(ValueError):
            s.solve_batch_compact_mixed(np.full(N + 1, H, dtype=np.int32), a["v"], a["dy"], a["dphi"])
        for call in (lambda: s.solve_batch_compact(a["v"], a["dy"], a["dphi"]),
                     lambda: s.solve_batch_compact_mixed(a["horizons"], a["v"], a["dy"], a["dphi"])):
            with pytest.raises(capi.TpcMpcError):   # accepted by the wrapper; the library has no device to run it on
                call()


def test_compact_vector_lengths_are_checked():
    """delta_y / delta_phi of another length than v: rejected by the wrapper (before the helper the three forward
    compact entries handed their addresses to C unchecked on the numpy side)"""
    a = base()
    long, short = np.zeros(N + 1), np.zeros(N - 1)
    with MpcSolver(horizon=H, device=None) as s:
        for bad in (long, short):
            for args in ((a["v"], bad, a["dphi"]), (a["v"], a["dy"], bad)):
                with pytest.raises(ValueError):
                    s.solve_batch_compact(*args)
                with pytest.raises(ValueError):
                    s.solve_batch_compact_exact(*args, fallback="none")
                with pytest.raises(ValueError):
                    s.solve_batch_compact_mixed(a["horizons"], *args)


# ---- the helper alone: no library (imported inside the tests: all of the above also runs on the code before it) ----

def test_arrays_read_coerces_and_keeps_alive():
    from trajectory_controller_amd._arrays import Arrays
    ar = Arrays(np.zeros((4, N)), N)
    assert ar.mem == capi.HOST and ar.stream is None and ar.n == N and ar.keep == []
    x = np.arange(2.0 * N).reshape(2, N)
    assert ar.read(None, 2) is None and ar.keep == []
    assert ar.read(x, 2) == x.ctypes.data and ar.keep[-1] is x          # already right: no copy
    for other in (x.astype(np.float32), np.ascontiguousarray(x.T).T, x.tolist()):
        addr = ar.read(other, 2)
        kept = ar.keep[-1]
        assert kept is not other and kept.ctypes.data == addr and kept.flags.c_contiguous
        assert kept.dtype == np.float64 and np.array_equal(kept, x)
    assert len(ar.keep) == 4
    st = ar.read([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.int32)
    assert ar.keep[-1].dtype == np.int32 and ar.keep[-1].ctypes.data == st
    for bad, rows in ((x, 3), (x, None), (np.zeros(N + 1), None), (np.zeros((2, N + 1)), 2)):
        with pytest.raises(ValueError):
            ar.read(bad, rows)


def test_arrays_loose_and_length_only():
    from trajectory_controller_amd._arrays import Arrays
    ar = Arrays(np.zeros(N))                      # n from the first array's element count
    assert ar.n == N
    t = np.zeros((K, 3, N))
    assert ar.read(t, K * 3, match="loose") == t.ctypes.data
    assert ar.read(np.zeros((3, N)), 3, match="loose") and ar.read(np.zeros(3 * N).reshape(3, 1, N), 3, match="loose")
    for bad in (np.zeros((K, 4, N)), np.zeros((N, 3 * K)), np.zeros(K * 3 * N + 1)):
        with pytest.raises(ValueError):
            ar.read(bad, K * 3, match="loose")
    with pytest.raises(ValueError):
        ar.read(t, K * 3)                         # the exact shape is [rows, n]
    assert ar.read(np.zeros((N, 1)), match="length") and ar.read(np.zeros((2, N // 2)), match="length")
    for bad in (np.zeros(N + 1), np.zeros(N - 1), np.zeros((2, N))):
        with pytest.raises(ValueError):
            ar.read(bad, match="length")


def test_arrays_update_is_strict():
    from trajectory_controller_amd._arrays import Arrays
    ar = Arrays([[0.0] * N] * 4, N)
    x = np.zeros((2, N))
    assert ar.update(None, 2) is None
    assert ar.update(x, 2) == x.ctypes.data and ar.keep == []
    for bad in (x.astype(np.float32), np.zeros((N, 2)).T, x.tolist(), np.zeros((3, N)), np.zeros(N)):
        with pytest.raises(ValueError):
            ar.update(bad, 2)
    i = np.zeros(N, dtype=np.int32)
    assert ar.update(i, dtype=np.int32) == i.ctypes.data
    with pytest.raises(ValueError):
        ar.update(i)


def test_arrays_new_and_addr():
    from trajectory_controller_amd._arrays import Arrays
    for dtype, np_dtype in ((capi.F64, np.float64), (capi.F32, np.float32), (np.float64, np.float64)):
        ar = Arrays(np.zeros((4, N)), N, dtype)
        a, b, c, d = ar.new(), ar.new(3), ar.new(K, 3), ar.new(10, per_instance=False)
        assert [x.shape for x in (a, b, c, d)] == [(N,), (3, N), (K, 3, N), (10,)]
        assert all(x.dtype == np_dtype and x.flags.c_contiguous for x in (a, b, c, d))
        assert ar.new(S, dtype=np.int32).dtype == np.int32
        assert ar.addr(None) is None and ar.addr(b) == b.ctypes.data


def test_arrays_address_of_read_only_and_empty_arrays():
    from trajectory_controller_amd._arrays import Arrays, _address
    for x in (np.arange(6.0).reshape(2, 3), np.zeros(0), np.arange(4, dtype=np.int32)):
        ro = x.copy()
        ro.flags.writeable = False
        assert _address(x) == x.ctypes.data and _address(ro) == ro.ctypes.data
    ar = Arrays(np.zeros(3), 3)
    ro = np.arange(6.0).reshape(2, 3)
    ro.flags.writeable = False
    assert ar.read(ro, 2) == ro.ctypes.data and ar.read_rows((ro, None), (2, 2)) == [ro.ctypes.data, None]
