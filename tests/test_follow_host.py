"""The float32 reference of the raw-trajectory entries (tests/model/follow_ref.py), held on the CPU to what defines this
build's geometry: the module shim's getTrajectoryPoint, vertex2f and LookupTable::linearSearch, called by
tests/host/follow_harness.cpp on a host-only solver handle.  Everything is compared bit for bit.

Also here, from the reference alone: the independent-walk horizon reference against the single pass it replaces, and the
conditions that make the edge batches worth running on the GPU (tests/test_follow_gpu.py), so none of them passes
vacuously."""
import os
import subprocess

import numpy as np
import pytest

from conftest import bits_equal32
from tests.model import follow_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "trajectory_controller_amd", "host")
LIB = os.path.join(ROOT, "trajectory_controller_amd", "lib")
N_EDGE = 130                      # columns of the edge batches here (every case at least once)
TABLE_NAMES = list(fr.TABLES)
POINT_KEYS = ("ox", "oy", "odx", "ody", "ovel", "dist")


def _batches():
    out = {name: build(N_EDGE) for name, build in fr.EDGE_BUILDERS.items()}
    out["random"] = fr.random_batch(2000, 24, 5)
    return out


@pytest.fixture(scope="module")
def batches():
    return _batches()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = str(tmp_path_factory.mktemp("follow") / "follow_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(HOST, "lms_compat"), "-I" + HOST,
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "follow_harness.cpp"),
                           "-o", exe, "-L" + LIB, "-ltrajectory_point_controller", "-ltpc_mpc", "-Wl,-rpath," + LIB])
    return exe


def _shim(exe, tmp_path, b, cols):
    """The shim's answers for columns `cols` of batch b: float32 [len(cols), 6 + tables]."""
    words = [float(len(TABLE_NAMES))]
    for name in TABLE_NAMES:
        vx, vy = fr.TABLES[name] if fr.TABLES[name] is not None else ((), ())
        words += [float(len(vx)), *map(float, vx), *map(float, vy)]
    words.append(float(len(cols)))
    for k in cols:
        cnt = int(b["count"][k])
        words += [float(cnt), b["look"][k], b["carv"][k]]
        for i in range(max(cnt, 0)):
            words += [b[name][i, k] for name in ("px", "py", "dx", "dy", "vel")]
    path = tmp_path / "cases.bin"
    np.asarray(words, dtype=np.float32).tofile(path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [[float.fromhex(tok) for tok in line.split()] for line in r.stdout.splitlines()]
    assert len(rows) == len(cols)
    got = np.asarray(rows, dtype=np.float64)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got, equal_nan=True)      # floats, printed exactly
    return got.astype(np.float32)


def _no_stop_point(b):
    """Columns the shim's crossing-stop PID (:445-473, not part of the batched entries) leaves alone: no point of the
    trajectory has velocity 0."""
    P, n = b["px"].shape
    used = np.arange(P)[:, None] < b["count"][None, :]
    return np.flatnonzero(~np.any(used & (b["vel"] == 0), axis=0))


@pytest.mark.parametrize("name", list(fr.EDGE_BUILDERS) + ["random"])
def test_reference_equals_the_shim(harness, tmp_path, batches, name):
    """follow_ref's point, target distance and model speed equal the shim's bit for bit -- the scalar definition and the
    batched form both, on every edge batch and 2000 random polylines."""
    b = batches[name]
    cols = _no_stop_point(b)
    assert len(cols) >= (0.6 if name in ("random", "crossing") else 0.99) * len(b["count"])
    got = _shim(harness, tmp_path, b, cols)
    traj = [b[k] for k in ("px", "py", "dx", "dy", "vel")]
    ref = fr.traj_points(*traj, b["count"], b["look"])
    for j, key in enumerate(POINT_KEYS):
        assert bits_equal32(ref[key][cols], got[:, j]), (name, key)
    for j, tname in enumerate(TABLE_NAMES):
        tab = fr.TABLES[tname] or (None, None)
        assert bits_equal32(fr.lut_batch(b["carv"], *tab)[cols], got[:, 6 + j]), (name, tname)
    # the scalar definition (plain loops) on a share of the columns
    row = {k: i for i, k in enumerate(cols)}
    for k in cols[:400]:
        one = fr.traj_point(*[a[:, k] for a in traj], int(b["count"][k]), b["look"][k])
        assert bits_equal32(np.array(one), got[row[k], :6]), (name, k)
        for j, tname in enumerate(TABLE_NAMES):
            tab = fr.TABLES[tname] or (None, None)
            assert bits_equal32(fr.lut(b["carv"][k], *tab), got[row[k], 6 + j]), (name, tname, k)


@pytest.mark.parametrize("name", list(fr.EDGE_BUILDERS) + ["random"])
def test_scalar_and_batched_reference_agree(batches, name):
    """Also where the shim cannot be asked (a trajectory point with velocity 0 starts its stateful crossing-stop PID):
    the batched reference equals the scalar one on every column, horizon steps included."""
    b = batches[name]
    n = min(len(b["count"]), 300)
    traj = [b[k][:, :n] for k in ("px", "py", "dx", "dy", "vel")]
    H = 7
    spacing = b["spacing"][:n] if b["spacing"] is not None else fr.default_spacing(fr.lut_batch(b["carv"][:n]), 0.1)
    steps = fr.horizon_batch(*traj, b["count"][:n], b["look"][:n], spacing, H)
    for k in range(n):
        one = fr.horizon_points(*[a[:, k] for a in traj], int(b["count"][k]), b["look"][k], spacing[k], H)
        for t in range(H):
            assert bits_equal32(np.array(one[t]), np.array([steps[t][key][k] for key in POINT_KEYS])), (name, k, t)


def test_spacing_zero_repeats_the_point(batches):
    for name, b in batches.items():
        traj = [b[k] for k in ("px", "py", "dx", "dy", "vel")]
        one = fr.traj_points(*traj, b["count"], b["look"])
        for s in fr.horizon_batch(*traj, b["count"], b["look"], np.zeros_like(b["look"]), 5):
            assert all(bits_equal32(s[key], one[key]) for key in POINT_KEYS), name


def test_independent_walks_equal_the_single_pass_for_growing_distances(batches):
    """Only the reference changed, not the expectation: for spacing >= 0 H independent walks give what the single pass
    of the first horizon test gave, on the random batch (the default spacing and a drawn one)."""
    b = batches["random"]
    n, H = 600, 10
    traj = [b[k][:, :n] for k in ("px", "py", "dx", "dy", "vel")]
    drawn = np.random.default_rng(3).uniform(0.0, 0.4, size=n).astype(np.float32)
    for spacing in (fr.default_spacing(fr.lut_batch(b["carv"][:n]), 0.1), drawn):
        assert np.all(spacing >= 0)
        steps = fr.horizon_batch(*traj, b["count"][:n], b["look"][:n], spacing, H)
        for k in range(n):
            old = fr.walk_single_pass(*[a[:, k] for a in traj], int(b["count"][k]), b["look"][k], spacing[k], H)
            for t in range(H):
                assert bits_equal32(np.array(old[t]), np.array([steps[t][key][k] for key in POINT_KEYS[:5]])), (k, t)


def test_negative_spacing_is_walked_not_extrapolated(batches):
    """What the single pass did with shrinking distances: steps t >= 1 extrapolated backwards along the segment that holds
    step 0's point -- the same point as long as the step stays inside that segment, another one once it leaves it.  The
    independent walks differ from the single pass on at least a quarter of the negative-spacing columns: the case exists."""
    b = batches["spacing"]
    traj = [b[k] for k in ("px", "py", "dx", "dy", "vel")]
    neg = np.flatnonzero(b["spacing"] < 0)
    assert len(neg) >= 0.2 * len(b["spacing"])
    H = 10
    steps = fr.horizon_batch(*traj, b["count"], b["look"], b["spacing"], H)
    differ = 0
    for k in neg:
        old = fr.walk_single_pass(*[a[:, k] for a in traj], int(b["count"][k]), b["look"][k], b["spacing"][k], H)
        differ += any(not bits_equal32(np.array(old[t][:2]), np.array([steps[t]["ox"][k], steps[t]["oy"][k]])) for t in range(H))
    assert differ >= 0.25 * len(neg), (differ, len(neg))


def test_edge_batches_cover_their_edges(batches):
    """Computed from the reference alone, asserted: a GPU test on these batches cannot pass vacuously."""
    H = 10
    walk = lambda b, want: fr.traj_points(*[b[k] for k in ("px", "py", "dx", "dy", "vel")], b["count"], want)
    # ties: the look-ahead exactly on a point's arc length, the last point's included; and horizon steps on points
    b = batches["tie"]
    one = walk(b, b["look"])
    assert one["tie"].mean() >= 0.25
    assert np.any(one["tie"] & (one["seg"] == fr.LAST)) and np.any(one["tie"] & (one["seg"] >= 1))
    steps = fr.horizon_batch(*[b[k] for k in ("px", "py", "dx", "dy", "vel")], b["count"], b["look"], b["spacing"], H)
    step_ties = np.sum([s["tie"] for s in steps[1:]], axis=0)
    assert (step_ties >= 2).mean() >= 0.25
    # `>=` would take the neighbour's vel: the crossing decision hangs on the tie in a good share of the batch
    P, n = b["px"].shape
    on = np.flatnonzero(one["tie"] & (one["seg"] >= 1))
    other = b["vel"][one["seg"][on] - 1, on]
    assert np.mean((other < 0.5) != (one["ovel"][on] < 0.5)) >= 0.5
    # the horizon edge batch (and the tie batch): several steps inside one segment, steps past the end
    for name in ("tie", "spacing"):
        b = batches[name]
        steps = fr.horizon_batch(*[b[k] for k in ("px", "py", "dx", "dy", "vel")], b["count"], b["look"], b["spacing"], H)
        seg = np.stack([s["seg"] for s in steps])                      # [H, n]
        shared = np.array([np.max(np.bincount(col[col >= 1], minlength=2)) >= 2 if np.any(col >= 1) else False for col in seg.T])
        assert shared.mean() >= 0.25, name
        assert np.any(seg == fr.LAST, axis=0).mean() >= (0.25 if name == "spacing" else 0.10), name
    # degenerate: every kind is there
    b = batches["degenerate"]
    one = walk(b, b["look"])
    P, n = b["px"].shape
    used = (np.arange(1, P)[:, None] < b["count"][None, :])
    zero_len = used & (b["px"][1:] == b["px"][:-1]) & (b["py"][1:] == b["py"][:-1])
    assert zero_len.any(axis=0).mean() >= 0.25
    for cnt in (0, 1, 2):
        assert np.any(b["count"] == cnt)
    assert np.any(b["count"] < 0) and np.any(one["seg"] == fr.NOTHING)
    assert np.any(b["look"] == 0) and np.any(b["look"] < 0) and np.any(one["seg"] == fr.LAST)
    hit = one["seg"] >= 1
    first_zero = zero_len[0] & (b["look"] < 0)                          # back > 0 on a zero-length first segment
    assert np.any(first_zero & (one["seg"] == 1))
    assert np.any(np.signbit(b["look"]) & (b["look"] == 0))
    assert hit.mean() >= 0.25
    # crossing rule: both sides, and the values next to 0.5
    b = batches["crossing"]
    ts = walk(b, b["look"])["ovel"]
    assert (ts < 0.5).mean() >= 0.10 and (~(ts < 0.5)).mean() >= 0.10
    half = np.float32(0.5)
    for val in (half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)), np.float32(0)):
        assert np.any(ts == val)
    assert np.any(ts < 0)
    # speeds: both sides of the clamp, the clamp's edge, every knot of every table, beyond both ends
    b = batches["speed"]
    v = b["carv"].astype(np.float64)
    assert np.any(np.abs(v) < 0.1) and np.any(v == np.float64(np.float32(0.1))) and np.any(v == -np.float64(np.float32(0.1)))
    assert np.any(v == 0)
    x = fr.lut_batch(b["carv"])
    for name, tab in fr.TABLES.items():
        if tab is None:
            continue
        vx = tab[0]
        for knot in vx:
            assert np.any(x == knot), (name, knot)
        assert np.any(x < vx[0]), name
        assert np.any(x > vx[-1]), name
    # spacing kinds
    sp = batches["spacing"]["spacing"]
    assert np.any(sp == 0) and np.any(sp < 0) and np.any((sp > 0) & (sp < 1e-3)) and np.any(sp >= 2)
