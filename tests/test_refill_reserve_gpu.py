"""The refill pass of the hand-written fp64 N = 20 projected-gradient kernel (mpc_ub_pg_asm.h) at the queue lengths where its
ticket handling can go wrong, on pinned grids of 1 and 3 wavefronts against the CPU model, as in tests/test_refill_gpu.py:
outputs and iteration counts bit for bit.

WHAT RUNS.  Every GPU test here runs the COMMITTED header: the refill threshold chosen by queue position (scripts/
gen_ub_pg_asm.py, SCHED: kUbAsmBatch / kUbAsmSchedMid / kUbAsmSchedLate lanes, read from the header below) and, while
kUbAsmReserve is absent from it, every pass drawing its own tickets.  The generator's draw-ahead mode (RESERVE) is off in the
shipped header, so none of these tests runs it; the sizes and cases are the ones at which it could go wrong, and hold for
whatever header is committed (the module reads the thresholds and the mode from it).
WHAT THEY HOLD.  Bits, counts, flags and termination.  Outputs do not depend on which lane solves an instance, so a wrong
threshold VALUE would still pass: the values are held by tests/test_build_artifacts.py (header = generator's output) and were
chosen by the A/B in profiles/r22_refill_reserve_ab.txt.

The QUEUE is what enters the projected-gradient phase (the model's count > smo_iters), not the batch: every batch here is
`nq` instances of a stream that the model takes into that phase plus a few that it does not, in the stream's order.  With
L = 64 x wavefronts lanes and B each threshold of the shipped header, nq is
  L - 7                       every ticket after the first pass's is past the end;
  L                           the first pass takes the queue exactly;
  L + 1, L + B - 1, L + B, L + B + 1   the last in-range ticket sits in the second pass, alone / last / one short;
  2 L + 1;
  6 L + 5                     both position thresholds are crossed: all three threshold values are in force in turn.
Further: equal instances (all 64 lanes of a wavefront stop in the same iteration: 64 lanes wait where the threshold is 3 to
8), and max_iter reached next to passes.  The non-finite case exercises NOTHING of the hand-written kernel but its launch:
the screen refuses a batch with non-finite inputs, the kernel returns at once and the exact build answers; it is
tests/test_refill_gpu.py's poisoning at these lengths, kept so that the early return is seen with this header too.

Host tests (no GPU): scripts/probes/queue_full_sim.py's "every queue entry served exactly once" on the same queue lengths
and counts, for every draw mode the simulator knows.
"""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, bits_equal
from test_refill_gpu import LANE_FMA, NTHREADS, WAVE, _compact_dev, _pin, _solver

H = 20
SMO = 50
FIRST = 3000                 # tests/test_refill_gpu.py's stream for N = 20: nearly every instance enters the projected-gradient phase
POOL = 4000
GRIDS = [1, 3]


def _shipped():
    """(thresholds in use, draw mode) of the committed header"""
    text = open(os.path.join(ROOT, "trajectory_controller_amd", "csrc", "mpc_ub_pg_asm.h")).read()
    num = lambda name, default: int(m.group(1)) if (m := re.search(rf"\b{name} = (\d+)", text)) else default
    b0 = num("kUbAsmBatch", None)
    return (b0, num("kUbAsmSchedMid", b0), num("kUbAsmSchedLate", b0)), ("off", "pass_end", "due")[num("kUbAsmReserve", 0)]


SCHED, MODE = _shipped()


def _queue_lengths(W):
    L = WAVE * W
    s = {L - 7, L, L + 1, 2 * L + 1, 6 * L + 5}
    for b in SCHED:
        s |= {L + b - 1, L + b, L + b + 1}
    return sorted(s)


@pytest.fixture(scope="module")
def model():
    from tests.model.bindings import UbModel
    return UbModel()


@pytest.fixture(scope="module")
def pool(model):
    """the stream and the model's answers for it, computed once: (v, dy, dphi), (front, rear, iters)"""
    from trajectory_controller_amd.synth import compact_inputs
    inp = compact_inputs(H, POOL, first=FIRST)
    mf, mr, mit, _ = model.solve_compact(H, *inp, nthreads=NTHREADS)
    return inp, (mf, mr, mit)


def _batch(mit, nq, smo=SMO, others=5):
    """indices into the pool: the first nq instances that enter the projected-gradient phase and the first `others` that do not"""
    enter, rest = np.flatnonzero(mit > smo), np.flatnonzero(mit <= smo)
    assert len(enter) >= nq, (len(enter), nq)
    return np.sort(np.concatenate([enter[:nq], rest[:others]]))


def _sim():
    sys.path.insert(0, os.path.join(ROOT, "scripts", "probes"))
    import queue_full_sim
    return queue_full_sim


# ---------------------------------------------------------------------------------------------
# host: the simulator's bookkeeping on these queue lengths

@pytest.mark.parametrize("W", GRIDS)
@pytest.mark.parametrize("mode", ["off", "pass_end", "first_stop", "due"])
def test_sim_serves_every_entry_once(pool, W, mode):
    sim = _sim()
    mit = pool[1][2]
    for nq in _queue_lengths(W):
        work = mit[np.flatnonzero(mit > SMO)[:nq]] - SMO
        for topup in ([False, True] if mode in ("pass_end", "first_stop") else [False]):
            out = sim.simulate(work, waves=W, sched=SCHED, reserve=mode, reserved_cost=1.0, topup=topup)   # (asserts)
            assert out["wave_iterations"] >= int(work.max()), (nq, out)
    same = np.full(4 * WAVE * W + 5, 77)                                 # every lane of a wavefront stops in the same iteration
    sim.simulate(same, waves=W, sched=SCHED, reserve=mode, reserved_cost=1.0)


# ---------------------------------------------------------------------------------------------
# GPU

@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _hold(torch, s, inp, ref, idx, what):
    v, dy, dphi = (np.ascontiguousarray(a[idx]) for a in inp)
    f, r, it = _compact_dev(torch, s, v, dy, dphi, LANE_FMA)
    assert np.array_equal(it, ref[2][idx]), what
    assert bits_equal(f, ref[0][idx]) and bits_equal(r, ref[1][idx]), what


@pytest.mark.gpu
@pytest.mark.parametrize("W", GRIDS)
def test_refill_threshold_queue_lengths(torch_cuda, pool, W):
    inp, ref = pool
    L = WAVE * W
    with _solver(H, "lane_fma") as s:
        _pin(s, W)
        for nq in _queue_lengths(W):
            _hold(torch_cuda, s, inp, ref, _batch(ref[2], nq), (W, nq))
            wave_iters, passes = s.last_lane_stats()
            print(f"W={W} queue {nq}: {wave_iters} wave iterations, {passes} refill passes, shipped thresholds {SCHED} draw mode {MODE}")
            assert passes >= W
            if nq > 6 * L:
                assert passes > 3 * W, (nq, passes)      # every lane refilled several times


@pytest.mark.gpu
@pytest.mark.parametrize("W", GRIDS)
def test_refill_equal_instances_stop_together(torch_cuda, pool, W):
    """One instance 4 L + 5 times: all 64 lanes of a wavefront stop in the same iteration, so a pass finds 64 lanes waiting
    where its threshold is 3 to 8, and the queue ends inside such a pass."""
    inp, ref = pool
    mit = ref[2]
    j = int(np.flatnonzero((mit > SMO + 10) & (mit < 400))[0])
    idx = np.full(4 * WAVE * W + 5, j)
    with _solver(H, "lane_fma") as s:
        _pin(s, W)
        _hold(torch_cuda, s, inp, ref, idx, (W, j))
        assert s.last_lane_stats()[1] > W


@pytest.mark.gpu
@pytest.mark.parametrize("W", GRIDS)
def test_refill_cap_next_to_passes(torch_cuda, model, pool, W):
    """max_iter = 300: lanes reach the cap next to passes (tests/test_refill_gpu.py's (50, 300)), at 4 L + 37 and at L + B
    queue entries (B: the late threshold); FLAG_MAX_ITER follows the model's counts."""
    from trajectory_controller_amd import FLAG_MAX_ITER
    inp = tuple(a[:1500] for a in pool[0])
    mf, mr, mit, _ = model.solve_compact(H, *inp, nthreads=NTHREADS, smo_iters=SMO, max_iter=300)
    assert (mit == 300).any() and (mit < 300).any()
    L = WAVE * W
    with _solver(H, "lane_fma", smo_iters=SMO, max_iter=300) as s:
        _pin(s, W)
        for nq in (L + SCHED[-1], 4 * L + 37):
            idx = _batch(mit, nq)
            _hold(torch_cuda, s, inp, (mf, mr, mit), idx, (W, nq))
            assert bool(s.last_flags & FLAG_MAX_ITER) == bool((mit[idx] == 300).any()), nq


@pytest.mark.gpu
@pytest.mark.parametrize("W", GRIDS)
def test_refill_nonfinite_inputs_divert_the_batch(torch_cuda, model, pool, W):
    """(the hand-written kernel only returns at once here: module docstring)"""
    from trajectory_controller_amd import FLAG_NONFINITE
    L = WAVE * W
    with _solver(H, "lane_fma") as s:
        _pin(s, W)
        for nq in (L + SCHED[0], 4 * L + 37):
            idx = _batch(pool[1][2], nq)
            v, dy, dphi = (np.ascontiguousarray(a[idx]).copy() for a in pool[0])
            bad = [5, len(idx) - 4, len(idx) // 2]
            dy[bad[0]], v[bad[1]], dphi[bad[2]] = np.nan, np.inf, -np.inf
            mf, mr, mit, _ = model.solve_compact(H, v, dy, dphi, nthreads=NTHREADS, fast_stop=None)
            f, r, it = _compact_dev(torch_cuda, s, v, dy, dphi, LANE_FMA)
            assert np.array_equal(it, mit) and bits_equal(f, mf) and bits_equal(r, mr), (W, nq)
            assert np.all(f[bad] == 0) and np.all(r[bad] == 0) and np.all(it[bad] == 0) and s.last_flags & FLAG_NONFINITE, (W, nq)
