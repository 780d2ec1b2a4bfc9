#!/usr/bin/env python3
"""Probe (CPU): the persistent queue of the fp64 N = 20 projected-gradient kernel at FULL size -- 1 024 wavefronts x 64
lanes, all 262 144 instances of the headline stream, iteration counts from the checker in oracle/, queue order from the
committed table's key (gen_queue_key_table.predict), longest first.  scripts/probes/queue_key_sim.py runs every 16th
instance on 16 wavefronts: 16 instances per lane where the real batch has 4, which understates everything that happens at
the end of the queue; its "variants within 1 %" does not hold here.

Time is counted in wave iterations (event-driven: one event per ticket draw and per refill pass, in time order, so the ONE
ticket counter is read in the order the wavefronts reach it).  A wavefront iterates until `batch` of its lanes wait (or none
has work), then runs a refill pass that stalls it for `pass_cost` iterations.

    python scripts/probes/queue_full_sim.py [--sched 3,5,8] [--pct 60,85] [--pass-cost 2] [--reserve MODE] [--reserved-cost 1]
                                            [--topup] [--reserve-pct P] [--n 262144] [--waves 1024] [--table]

  --sched b0,b1,b2   refill threshold while the pass's first ticket is below pct[0] % / pct[1] % of the queue / beyond
  --reserve MODE     when the tickets of a pass are drawn (gen_ub_pg_asm.py's RESERVE):
       off           by the pass itself, as many as lanes wait (the pass waits for the atomic: pass_cost)
       pass_end      at the END of the pass before (64 at the start), as many as the next pass's threshold.  The wavefront
                     HOLDS them until its next pass, and that is what this models: a wavefront whose lanes run long
                     instances sits on tickets of long instances while wavefronts with idle lanes draw later, shorter ones
       first_stop    the same, drawn when the first lane stops after a pass
       due           when the pass falls due, as many as lanes wait; the wavefront runs ONE more iteration under the
                     atomic's round trip, then the pass (at reserved_cost) serves the reserved tickets; held for one iteration
  --topup            pass_end / first_stop: a pass with more waiting lanes than reserved tickets draws the difference at once
                     (at pass_cost) instead of leaving those lanes waiting
  --reserve-pct P    pass_end / first_stop: reserve only while the wavefront's latest first ticket is below P % of the queue
Prints makespan, wave iterations, passes per wavefront, lane utilisation; asserts that every queue entry is served exactly
once (simulate() is importable: tests/test_refill_reserve_gpu.py runs that assertion on its own queue lengths).
"""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WAVE = 64
MODES = ("off", "pass_end", "first_stop", "due")


def simulate(work, waves=1024, sched=(3, 3, 3), pct=(60, 85), pass_cost=2.0, reserve="off", reserved_cost=None, topup=False,
             reserve_pct=100):
    """work: projected-gradient iterations of the queue's entries, in queue order (all >= 1).  Returns a dict.
    pass_cost: iterations a pass stalls its wavefront for when it waits for a ticket draw; reserved_cost (default: the same):
    when its tickets were drawn most of an iteration earlier."""
    assert reserve in MODES
    reserved_cost = pass_cost if reserved_cost is None else reserved_cost
    work = np.asarray(work, dtype=np.int64)
    assert work.ndim == 1 and (work >= 1).all()
    nq = len(work)
    thr = (nq * pct[0] // 100, nq * pct[1] // 100)
    rem = np.zeros((waves, WAVE), dtype=np.int64)          # iterations a lane still has to run (0: no instance)
    exh = np.zeros((waves, WAVE), dtype=bool)
    batch = [sched[0]] * waves
    res = [None] * waves                                   # (first ticket, count, time drawn) held by the wavefront
    last_first = [0] * waves                               # first ticket of the wavefront's latest pass
    wave_iters = np.zeros(waves, dtype=np.int64)
    passes = np.zeros(waves, dtype=np.int64)
    end = np.zeros(waves)
    served = np.zeros(nq, dtype=np.int64)
    counter = 0
    DRAW, PASS = 0, 1                                      # (a draw comes before a pass at the same time)
    ev = []
    for w in range(waves):
        if reserve in ("pass_end", "first_stop"):
            ev.append((0.0, DRAW, w, WAVE))
        ev.append((0.0, PASS, w, 0))
    heapq.heapify(ev)

    def run_to_next_pass(w, t):
        """iterates wavefront w from time t until a pass is due; schedules it, or records the wavefront's end"""
        r = rem[w]
        have = r > 0
        want = int((~have & ~exh[w]).sum())
        nh = int(have.sum())
        if nh == 0 and want == 0:
            end[w] = t
            return
        k = k1 = 0
        if nh and want < batch[w]:
            s = np.sort(r[have])
            need = batch[w] - want
            k = int(s[need - 1] if need <= nh else s[-1])
            k1 = 0 if want else int(s[0])                  # the first lane to stop after the pass
            r[have] -= np.minimum(r[have], k)
            wave_iters[w] += k
        if reserve in ("pass_end", "first_stop") and last_first[w] < nq * reserve_pct // 100:
            heapq.heappush(ev, (t + (k1 if reserve == "first_stop" else 0), DRAW, w, batch[w]))
        if reserve == "due":
            have = r > 0
            if have.any():                                 # draw now, one more iteration, then the pass
                heapq.heappush(ev, (t + k, DRAW, w, int((~have & ~exh[w]).sum())))
                r[have] -= 1
                wave_iters[w] += 1
                k += 1
        heapq.heappush(ev, (t + k, PASS, w, 0))

    while ev:
        t, kind, w, cnt = heapq.heappop(ev)
        if kind == DRAW:
            res[w] = (counter, cnt, t)
            counter += cnt
            continue
        want = np.flatnonzero((rem[w] == 0) & ~exh[w])
        cost = pass_cost
        if res[w] is not None:
            first, n_res, drawn = res[w]
            res[w] = None
            if t - drawn >= 0.8:                           # (the atomic's round trip: ~1 770 of an iteration's ~2 200 cycles)
                cost = reserved_cost
            lanes = want[:n_res]                           # rank order; the rest stay waiting
            tickets = first + np.arange(len(lanes))
            # tickets reserved and not handed out are dropped: the served-exactly-once assertion holds them past the end
            if topup and len(want) > n_res:
                tickets = np.concatenate([tickets, counter + np.arange(len(want) - n_res)])
                counter += len(want) - n_res
                lanes, cost = want, pass_cost
        else:
            first = counter
            counter += len(want)
            lanes = want
            tickets = first + np.arange(len(lanes))
        last_first[w] = int(first)
        ok = tickets < nq
        served[tickets[ok]] += 1
        rem[w, lanes[ok]] = work[tickets[ok]]
        exh[w, lanes[~ok]] = True
        passes[w] += 1
        batch[w] = sched[0] if first < thr[0] else sched[1] if first < thr[1] else sched[2]
        run_to_next_pass(w, t + cost)
    assert (served == 1).all(), f"{int((served != 1).sum())} queue entries not served exactly once"
    total = int(wave_iters.sum())
    return {"makespan": float(end.max()), "wave_iterations": total, "passes_per_wavefront": float(passes.mean()),
            "utilisation": float(work.sum()) / (WAVE * total) if total else 0.0, "tickets_drawn": int(counter)}


def headline_queue(n, H=20, smo=50, nthreads=None):
    """the queue of the headline stream: projected-gradient iteration counts in the order of the table's key, longest first"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_queue_key_table as qk
    from oracle.bindings import Oracle
    from trajectory_controller_amd.synth import compact_inputs
    v, dy, dphi = compact_inputs(H, n)
    it = Oracle().solve_compact(H, v, dy, dphi, nthreads=nthreads or min(16, os.cpu_count() or 1))[2]
    table, _ = qk.load_header()
    key = qk.predict(table, v, dy, dphi).astype(np.float64)
    order = np.argsort(-key, kind="stable")
    order = order[it[order] > smo]
    return (it[order] - smo).astype(np.int64)


# (sched, pass_cost, reserve, reserved_cost, topup, reserve_pct): NOTEBOOK.md's table.  A reserved pass does not wait for its
# ticket, ~1 770 of a pass's ~4 000 cycles: about 1 iteration instead of 2
TABLE = [("3,3,3", 2.0, "off", None, False, 100), ("3,3,3", 1.0, "off", None, False, 100),
         ("3,5,8", 2.0, "off", None, False, 100), ("3,6,12", 2.0, "off", None, False, 100), ("6,6,6", 2.0, "off", None, False, 100),
         ("1,1,1", 0.0, "off", None, False, 100),
         ("3,3,3", 2.0, "pass_end", 1.0, False, 100), ("3,3,3", 2.0, "pass_end", 1.0, True, 100), ("3,3,3", 2.0, "pass_end", 1.0, False, 50),
         ("3,5,8", 2.0, "pass_end", 1.0, False, 100),
         ("3,3,3", 2.0, "first_stop", 1.0, False, 100), ("3,3,3", 2.0, "first_stop", 1.0, True, 100),
         ("3,3,3", 2.0, "due", 1.0, False, 100), ("3,5,8", 2.0, "due", 1.0, False, 100), ("3,6,12", 2.0, "due", 1.0, False, 100)]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sched", default="3,3,3")
    ap.add_argument("--pct", default="60,85")
    ap.add_argument("--pass-cost", type=float, default=2.0)
    ap.add_argument("--reserve", default="off", choices=MODES)
    ap.add_argument("--reserved-cost", type=float, default=None)
    ap.add_argument("--topup", action="store_true")
    ap.add_argument("--reserve-pct", type=int, default=100)
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--waves", type=int, default=1024)
    ap.add_argument("--table", action="store_true", help="the variants of NOTEBOOK.md's table on one queue, instead of one run")
    a = ap.parse_args()
    work = headline_queue(a.n)
    runs = TABLE if a.table else [(a.sched, a.pass_cost, a.reserve, a.reserved_cost, a.topup, a.reserve_pct)]
    for sched, cost, reserve, rcost, topup, rpct in runs:
        out = simulate(work, a.waves, tuple(int(c) for c in sched.split(",")), tuple(int(c) for c in a.pct.split(",")), cost, reserve,
                       rcost, topup, rpct)
        print(f"n {a.n} queue {len(work)} waves {a.waves} sched {sched} pct {a.pct} pass_cost {cost:g} reserve {reserve} "
              f"reserved_cost {cost if rcost is None else rcost:g} topup {int(topup)} reserve_pct {rpct}: "
              f"makespan {out['makespan']:.0f}  wave_iterations {out['wave_iterations']}  passes/wavefront {out['passes_per_wavefront']:.1f}  "
              f"utilisation {out['utilisation']:.3f}", flush=True)
