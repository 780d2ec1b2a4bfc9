"""float32 reference of the raw-trajectory entries' geometry (csrc/mpc_follow.hip) and the edge batches its tests run on.

The definition is the module shim: host/trajectory_point_controller.cpp::getTrajectoryPoint, lms_compat's
LookupTable::linearSearch and vertex2f (tests/test_follow_host.py holds this file to them bit for bit).  Every product and
sum is rounded to float32 one at a time -- the kernels are built with -ffp-contract=off, so the bits are the kernel's.

  traj_point / lut / horizon_points      one polyline, plain loops: the readable definition
  traj_points / lut_batch / horizon_batch    the same over a [P, n] batch, one numpy operation per scalar operation
                                             (equal to the scalar forms bit for bit: asserted in the host test)
  walk_single_pass                       the single-pass walk the first horizon test used (spacing >= 0 only)
  *_batch builders                       edge cases, SoA [P, n] float32 with ragged counts

The header defines horizon step t as "the polyline point at arc length look_ahead + t * spacing": H independent
getTrajectoryPoint walks.  horizon_points is exactly that, never a single pass.
"""
import numpy as np

f32 = np.float32
P_EDGE = 12          # rows of every edge batch (points beyond count[k] hold NaN: they must not be read)


# ---------------------------------------------------------------------------------------------
# one polyline

def traj_point(px, py, dx, dy, vel, count, want):
    """getTrajectoryPoint(want) on points [0, count): (ox, oy, odx, ody, ovel, |(ox, oy)|), all float32."""
    f = f32
    want = f(want)
    with np.errstate(all="ignore"):
        ox, oy, odx, ody, ovel = want, f(0), f(1), f(0), f(0)
        if count > 0:
            walked, found = f(0), False
            for i in range(1, count):
                ex, ey = f(px[i - 1] - px[i]), f(py[i - 1] - py[i])
                ln = f(np.sqrt(f(f(ex * ex) + f(ey * ey))))
                walked = f(walked + ln)
                if walked > want:
                    back = f(walked - want)
                    nx, ny = (f(ex / ln), f(ey / ln)) if ln > 0 else (f(0), f(0))
                    ox, oy = f(px[i] + f(nx * back)), f(py[i] + f(ny * back))
                    odx, ody, ovel, found = dx[i], dy[i], vel[i], True
                    break
            if not found:
                j = count - 1
                ox, oy, odx, ody, ovel = px[j], py[j], dx[j], dy[j], vel[j]
        return ox, oy, odx, ody, ovel, f(np.sqrt(f(f(ox * ox) + f(oy * oy))))


def step_want(first, spacing, t):
    """Arc length of horizon step t in the kernel's float32 operations: first, then first + float(t) * spacing."""
    with np.errstate(all="ignore"):
        return f32(first) if t == 0 else f32(f32(first) + f32(f32(t) * f32(spacing)))


def horizon_points(px, py, dx, dy, vel, count, first, spacing, H):
    """H independent getTrajectoryPoint walks: [(ox, oy, odx, ody, ovel, dist)] per step."""
    return [traj_point(px, py, dx, dy, vel, count, step_want(first, spacing, t)) for t in range(H)]


def clamp_speed(car_velocity):
    """cycle()'s |v| < 0.1 -> 0.1 in double, then the cast to the float the lookup table works in."""
    v = np.float64(car_velocity)
    if abs(v) < 0.1:
        v = np.float64(0.1)
    return f32(v)


def lut(car_velocity, vx=None, vy=None):
    """The model's speed: clamp, then LookupTable<float>::linearSearch (no table: the clamped speed).  float32."""
    f = f32
    x = clamp_speed(car_velocity)
    if vx is None or len(vx) == 0:
        return x
    if x <= vx[0]:
        return f(vy[0])
    with np.errstate(all="ignore"):
        for i in range(1, len(vx)):
            if x <= vx[i]:
                t = f(f(x - vx[i - 1]) / f(vx[i] - vx[i - 1]))
                return f(vy[i - 1] + f(t * f(vy[i] - vy[i - 1])))
    return f(vy[-1])


def default_spacing(v, step):
    """(float)(|v| * step_size): the distance driven per step, v the model's speed as a double."""
    return f32(np.abs(np.asarray(v, dtype=np.float64)) * np.float64(step))


def compact_model(v, step, wheelbase):
    """A[4, n], B[4, n] of the compact model in the kernel's operation order: av = step * v, cv = step * v / wheelbase."""
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    av = np.float64(step) * v
    cv = np.float64(step) * v / np.float64(wheelbase)
    one, zero = np.ones_like(v), np.zeros_like(v)
    return np.stack([one, av, zero, one]), np.stack([zero, av, cv, -cv])


def walk_single_pass(px, py, dx, dy, vel, count, first, spacing, H):
    """The single pass over the polyline that serves growing distances (spacing >= 0): per step
    (ox, oy, odx, ody, ovel).  Kept to show that for spacing >= 0 it and horizon_points agree."""
    f = np.float32
    out = []
    t = 0
    want = lambda t: f(first) if t == 0 else f(f(first) + f(f(t) * f(spacing)))
    if count > 0:
        walked = f(0)
        for i in range(1, count):
            if t >= H:
                break
            ex, ey = f(px[i - 1] - px[i]), f(py[i - 1] - py[i])
            ln = f(np.sqrt(f(f(ex * ex) + f(ey * ey))))
            walked = f(walked + ln)
            while t < H and walked > want(t):
                back = f(walked - want(t))
                nx, ny = (f(ex / ln), f(ey / ln)) if ln > 0 else (f(0), f(0))
                out.append((f(px[i] + f(nx * back)), f(py[i] + f(ny * back)), dx[i], dy[i], vel[i]))
                t += 1
        j = count - 1
        while t < H:
            out.append((px[j], py[j], dx[j], dy[j], vel[j]))
            t += 1
    else:
        while t < H:
            out.append((want(t), f(0), f(1), f(0), f(0)))
            t += 1
    return out


# ---------------------------------------------------------------------------------------------
# batches: the same operations, one numpy float32 array operation per scalar operation

NOTHING, LAST = -2, -1     # `seg` of traj_points: nothing to follow / fell through to the last point


def traj_points(px, py, dx, dy, vel, count, want, max_points=None):
    """traj_point for every column of [P, n] arrays.  Returns a dict of float32 [n] arrays ox, oy, odx, ody, ovel, dist,
    plus seg (the index of the segment end the point was taken from, LAST or NOTHING) and tie (the walked length
    equalled `want` exactly at some point that was compared)."""
    P, n = px.shape
    cnt = np.minimum(np.asarray(count, dtype=np.int64), P if max_points is None else max_points)
    want = np.asarray(want, dtype=f32)
    col = np.arange(n)
    with np.errstate(all="ignore"):
        ox, oy = want.copy(), np.zeros(n, f32)
        odx, ody, ovel = np.ones(n, f32), np.zeros(n, f32), np.zeros(n, f32)
        seg = np.full(n, NOTHING, dtype=np.int64)
        tie = np.zeros(n, dtype=bool)
        walked = np.zeros(n, f32)
        found = np.zeros(n, dtype=bool)
        for i in range(1, P):
            active = (i < cnt) & ~found
            if not active.any():
                break
            ex, ey = px[i - 1] - px[i], py[i - 1] - py[i]
            ln = np.sqrt(ex * ex + ey * ey)
            walked = np.where(active, walked + ln, walked)
            hit = active & (walked > want)
            tie |= active & (walked == want)
            back = walked - want
            pos = ln > 0
            nx = np.where(pos, ex / np.where(pos, ln, f32(1)), f32(0))
            ny = np.where(pos, ey / np.where(pos, ln, f32(1)), f32(0))
            ox = np.where(hit, px[i] + nx * back, ox)
            oy = np.where(hit, py[i] + ny * back, oy)
            odx, ody, ovel = np.where(hit, dx[i], odx), np.where(hit, dy[i], ody), np.where(hit, vel[i], ovel)
            seg = np.where(hit, i, seg)
            found |= hit
        last = (cnt > 0) & ~found
        j = np.clip(cnt - 1, 0, P - 1)
        ox, oy = np.where(last, px[j, col], ox), np.where(last, py[j, col], oy)
        odx, ody, ovel = np.where(last, dx[j, col], odx), np.where(last, dy[j, col], ody), np.where(last, vel[j, col], ovel)
        seg = np.where(last, LAST, seg)
        dist = np.sqrt(ox * ox + oy * oy)
    assert all(a.dtype == f32 for a in (ox, oy, odx, ody, ovel, dist))
    return dict(ox=ox, oy=oy, odx=odx, ody=ody, ovel=ovel, dist=dist, seg=seg, tie=tie)


def step_wants(first, spacing, t):
    first, spacing = np.asarray(first, dtype=f32), np.asarray(spacing, dtype=f32)
    with np.errstate(all="ignore"):
        return first.copy() if t == 0 else first + f32(t) * spacing


def horizon_batch(px, py, dx, dy, vel, count, first, spacing, H, max_points=None):
    """H independent traj_points walks.  Returns the list of their dicts, step 0 first."""
    return [traj_points(px, py, dx, dy, vel, count, step_wants(first, spacing, t), max_points) for t in range(H)]


def lut_batch(car_velocity, vx=None, vy=None):
    """lut() for an array of car velocities: float32 [n]."""
    v = np.asarray(car_velocity, dtype=np.float64).copy()
    v[np.abs(v) < 0.1] = 0.1
    x = v.astype(f32)
    if vx is None or len(vx) == 0:
        return x
    vx, vy = np.asarray(vx, dtype=f32), np.asarray(vy, dtype=f32)
    out = np.full(x.shape, vy[-1], dtype=f32)
    done = x <= vx[0]
    out[done] = vy[0]
    with np.errstate(all="ignore"):
        for i in range(1, len(vx)):
            m = ~done & (x <= vx[i])
            t = (x - vx[i - 1]) / (vx[i] - vx[i - 1])
            out = np.where(m, vy[i - 1] + t * (vy[i] - vy[i - 1]), out)
            done |= m
    assert out.dtype == f32
    return out


def targets_of(steps):
    """[2H, n] float64 targets of a horizon_batch result: row 2t = y, row 2t + 1 = phi (glibc's atan2)."""
    rows = []
    for s in steps:
        rows.append(s["oy"].astype(np.float64))
        rows.append(np.arctan2(s["ody"].astype(np.float64), s["odx"].astype(np.float64)))
    return np.stack(rows)


# ---------------------------------------------------------------------------------------------
# batches of cases

def random_trajectories(n, P, seed):
    """Smooth random polylines with ragged counts: the bulk case."""
    rng = np.random.default_rng(seed)
    seg = rng.uniform(0.02, 0.25, size=(P, n)).astype(np.float32)
    ang = np.cumsum(rng.uniform(-0.15, 0.15, size=(P, n)), axis=0).astype(np.float32)
    px = np.cumsum(seg * np.cos(ang), axis=0, dtype=np.float32)
    py = (np.cumsum(seg * np.sin(ang), axis=0, dtype=np.float32) + rng.uniform(-0.2, 0.2, size=n).astype(np.float32))
    dx, dy = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    vel = rng.uniform(0.0, 2.0, size=(P, n)).astype(np.float32)
    count = rng.integers(0, P + 1, size=n).astype(np.int32)
    count[:3] = (0, 1, 2)
    carv = rng.uniform(-0.2, 4.0, size=n).astype(np.float32)
    look = rng.uniform(0.2, 1.5, size=n).astype(np.float32)
    return px, py, dx, dy, vel, count, carv, look


FIELDS = ("px", "py", "dx", "dy", "vel", "count", "carv", "look")


def random_batch(n, P=24, seed=5):
    b = {k: np.ascontiguousarray(a[..., :n]) for k, a in zip(FIELDS, random_trajectories(max(n, 3), P, seed))}
    b["spacing"] = None
    return b


def _inst(points, look, carv=1.0, spacing=0.0, count=None):
    """One case: points [(x, y, dx, dy, vel)], the look-ahead, the car's speed, the step spacing, the count handed in."""
    return dict(points=[tuple(map(float, p)) for p in points], look=look, carv=carv, spacing=spacing,
                count=len(points) if count is None else count)


def pack(instances, n, P=P_EDGE):
    """Tile a list of cases to n columns of SoA [P, n] float32 arrays.  Rows a case does not own hold NaN."""
    assert instances and all(len(c["points"]) <= P for c in instances)
    arr = {k: np.full((P, n), np.nan, dtype=f32) for k in ("px", "py", "dx", "dy", "vel")}
    count, carv, look, spacing = np.zeros(n, np.int32), np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    for k in range(n):
        c = instances[k % len(instances)]
        for i, p in enumerate(c["points"]):
            for name, val in zip(("px", "py", "dx", "dy", "vel"), p):
                arr[name][i, k] = f32(val)
        count[k], carv[k], look[k], spacing[k] = c["count"], f32(c["carv"]), f32(c["look"]), f32(c["spacing"])
    return dict(arr, count=count, carv=carv, look=look, spacing=spacing)


def _polyline(segs, x0=0.0, y0=0.0, vels=None, scale=1.0):
    """Points from segment vectors; dir and vel differ from point to point."""
    pts, x, y = [], x0, y0
    for i in range(len(segs) + 1):
        if i:
            x, y = x + segs[i - 1][0] * scale, y + segs[i - 1][1] * scale
        a = 0.1 * i - 0.3
        v = vels[i % len(vels)] if vels else 0.6 + 0.1 * i
        pts.append((x, y, np.cos(a), np.sin(a), v))
    return pts


# segments whose lengths are exact in float32: 3-4-5 triangles over 16 and axis-aligned dyadic steps
_TIE_SEGS = [(3 / 16, 4 / 16), (4 / 16, 3 / 16), (4 / 16, 0.0), (0.0, 4 / 16), (3 / 16, -4 / 16), (8 / 16, 0.0), (6 / 16, 8 / 16)]
_TIE_LENS = [5 / 16, 5 / 16, 4 / 16, 4 / 16, 5 / 16, 8 / 16, 10 / 16]
_TIE_VELS = [0.25, 1.0, 0.375, 1.5, 0.125, 2.0, 0.4375, 0.75]     # neighbours sit on opposite sides of the crossing rule


def tie_batch(n):
    """Exact ties: every partial sum of the walk is exact in float32, and the look-ahead (and, for the horizon entry,
    first + t * spacing for several t) lies exactly on the arc length of a point -- the last one included.  `>=` in
    place of `>` takes the neighbouring point's dir and vel: another phi, target_speed and crossing decision."""
    cases = []
    for rot in range(4):
        for scale in (1.0, 2.0, 0.5):
            segs = _TIE_SEGS[rot:] + _TIE_SEGS[:rot]
            lens = _TIE_LENS[rot:] + _TIE_LENS[:rot]
            arc = np.cumsum([0.0] + [l * scale for l in lens])
            pts = _polyline(segs, x0=0.25 * rot, y0=-0.125 * rot, vels=_TIE_VELS[rot:] + _TIE_VELS[:rot], scale=scale)
            for i in (1, 2, 4, 7):                        # on point i; 7 is the last point
                cases.append(_inst(pts, arc[i], carv=1.0 + 0.25 * rot, spacing=scale / 16))        # steps on later points too
                cases.append(_inst(pts, arc[i] + scale / 32, carv=0.5 + rot, spacing=scale / 8))      # just past it
            for i in (1, 2, 3):
                cases.append(_inst(pts, arc[i], carv=1.5, spacing=scale / 8))
                cases.append(_inst(pts, arc[i] - scale / 16, carv=2.5, spacing=scale / 16))
            cases.append(_inst(pts, arc[3], carv=2.0, spacing=scale / 8))      # several steps inside the long segments
            cases.append(_inst(pts, arc[1] - scale / 32, carv=3.0, spacing=5 / 32 * scale))
    return pack(cases, n)


def degenerate_batch(n):
    """Zero-length segments, all points equal, count in {0, 1, 2, negative}, look-ahead 0, negative and beyond the end."""
    a, b, c, d = (0.1, 0.05), (0.37, 0.11), (0.52, 0.31), (0.9, 0.29)
    pt = lambda p, i: (p[0], p[1], np.cos(0.2 * i), np.sin(0.2 * i), 0.7 + 0.1 * i)
    poly = lambda ps: [pt(p, i) for i, p in enumerate(ps)]
    shapes = [
        poly([a, a, b, c, d]),            # duplicate at the start
        poly([a, a, a, b, c]),
        poly([a, b, b, c, d]),            # in the middle
        poly([a, b, c, c, c, d]),
        poly([a, b, c, d, d]),            # at the end
        poly([b, b, b, b, b]),            # all points equal
        poly([a, b, c, d]),               # nothing special: the look-aheads below make it a case
    ]
    cases = []
    for pts in shapes:
        for look in (0.0, -0.5, 0.3, 0.61, 25.0, -0.0):
            cases.append(_inst(pts, look, carv=1.3, spacing=0.11))
    full = poly([a, b, c, d])
    for cnt in (0, 1, 2, -3):
        for look in (0.0, 0.2, -0.5, 7.0):
            cases.append(_inst(full[:max(cnt, 0)], look, carv=0.9, spacing=0.2, count=cnt))
    cases.append(_inst(full[:0], 0.4, carv=1.0, spacing=np.inf, count=0))     # step 0 is `first`, whatever the spacing
    return pack(cases, n)


TABLES = {
    "none": None,
    "one": (np.array([1.0], f32), np.array([0.7], f32)),
    "four": (np.array([0.5, 1.0, 2.5, 4.0], f32), np.array([0.8, 1.0, 2.0, 2.4], f32)),
    "steep": (np.array([-1.0, 0.1, 0.3], f32), np.array([-0.6, 0.35, 3.1], f32)),
}
SPEEDS = [0.0, 0.05, -0.05, 0.1, -0.1, float(np.nextafter(f32(0.1), f32(0))), float(-np.nextafter(f32(0.1), f32(0))), -3.0,
          0.5, 1.0, 2.5, 4.0, 5.0, 0.3, -1.0, 0.7, 1.7, 3.3, 0.2, float(np.nextafter(f32(1.0), f32(2))),
          float(np.nextafter(f32(4.0), f32(5))), float(np.nextafter(f32(0.5), f32(0)))]


def speed_batch(n):
    """car_velocity on and around the clamp and on, between and beyond the knots of TABLES."""
    segs = [(0.11, 0.02), (0.13, -0.01), (0.09, 0.03), (0.2, 0.05), (0.17, -0.04), (0.12, 0.0)]
    cases = [_inst(_polyline(segs, y0=0.01 * i), 0.2 + 0.03 * i, carv=v, spacing=0.05) for i, v in enumerate(SPEEDS)]
    return pack(cases, n)


CROSSING_VELS = [0.5, float(np.nextafter(f32(0.5), f32(0))), 0.0, -1.0, 0.75, float(np.nextafter(f32(0.5), f32(1))), -0.0, 0.49]


def crossing_batch(n):
    """The chosen point's vel on, just below and just above 0.5, zero and negative."""
    segs = [(0.15, 0.02), (0.14, 0.04), (0.16, -0.03), (0.15, 0.0), (0.13, 0.05)]
    cases = []
    for i, v in enumerate(CROSSING_VELS):
        for look in (0.2, 0.45, 3.0):
            cases.append(_inst(_polyline(segs, y0=0.02 * i, vels=[v]), look, carv=0.8 + 0.2 * i, spacing=0.1))
    return pack(cases, n)


SPACINGS = [0.0, 1e-4, 5.0, 0.07, 0.02, 0.31, -0.05, -0.3, 0.011, 2.0, 0.045, -1e-3]


def spacing_batch(n):
    """The horizon entry's edge batch: spacing 0, tiny (all steps in one segment), large (steps 1.. past the end),
    ordinary and negative.  `spacing` is the per-instance array; passing None instead takes the |v| * step_size default."""
    segs = [(0.21, 0.03), (0.12, -0.02), (0.33, 0.06), (0.08, 0.01), (0.27, -0.05), (0.15, 0.02), (0.19, 0.0)]
    cases = []
    for i, sp in enumerate(SPACINGS):
        for look in (0.1, 0.5, 1.2):
            cases.append(_inst(_polyline(segs, y0=-0.01 * i), look, carv=0.4 + 0.3 * i, spacing=sp))
    return pack(cases, n)


EDGE_BUILDERS = {"tie": tie_batch, "degenerate": degenerate_batch, "speed": speed_batch, "crossing": crossing_batch,
                 "spacing": spacing_batch}


def concat(batches, P=24):
    """Batches side by side, padded with NaN rows to P points.  A batch without its own spacing gets the default
    (|v| * step_size with no lookup table, step_size 0.1)."""
    out = {}
    for k in ("px", "py", "dx", "dy", "vel"):
        out[k] = np.concatenate([np.concatenate([b[k], np.full((P - b[k].shape[0], b[k].shape[1]), np.nan, f32)]) for b in batches],
                                axis=1)
    for k in ("count", "carv", "look"):
        out[k] = np.concatenate([b[k] for b in batches])
    out["spacing"] = np.concatenate([b["spacing"] if b["spacing"] is not None else default_spacing(lut_batch(b["carv"]), 0.1)
                                     for b in batches])
    return out


def mixed_batch():
    """The bulk case and every edge batch in one: 1230 columns (no multiple of 64), what the composition tests solve."""
    return concat([random_batch(700, 24, 5), tie_batch(130), degenerate_batch(130), speed_batch(70), crossing_batch(70),
                   spacing_batch(130)])


def capped_batch(n, seed=9):
    """For the iteration cap: the bulk case with column k's lateral offsets and directions scaled by 10^-(k mod 5), so
    that at a small max_iter a good share of the instances ends on the cap and a good share does not."""
    b = random_batch(n, 24, seed)
    scale = (10.0 ** -(np.arange(n) % 5)).astype(f32)
    b["py"] = b["py"] * scale
    b["dy"] = b["dy"] * scale
    b["spacing"] = default_spacing(lut_batch(b["carv"]), 0.1)
    return b
