"""What q candidates per iteration cost: the time of a BO iteration at q = 1, 2, 4 in the headline
configuration (f15, d = 40, n_DoE 120, budget 450) early (n < 150) and late (n >= 400) in the run, split into the calls the
proposal loop makes - optimiser, extend, posterior, scoring - and the evaluations per second of the whole run; for a single PCA_BO
run and for a lock-step batch (--batch runs, acq_kernel "device").

Host clocks around calls that return after a wait on the stream (every library call timed here does; a batch's _begin / _end pair
is timed from the _begin to the return of the _end).  An iteration's time is the clock around `_bo_iteration` / `iteration()`: it
holds the objective's evaluations and the host's bookkeeping too, so the parts do not add up to it.  The q values are run in turn,
--rounds times; medians over a window's iterations, then the median of the rounds with their spread.  The first round warms every
shape.  No threshold.

usage: gpu_q_clock.py [--q 1 2 4] [--rounds 3] [--batch 30] [--no-single] [--no-batch] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.environ.get("PCABO_TREE", ROOT), "para-ortho-pca-bo_amd"))
from pcabo import _native as N                                      # noqa: E402
from pcabo.bbob import BBOBProblem                                  # noqa: E402

FID, DIM, BUDGET, NDOE = 15, 40, 450, 120
WINDOWS = {"n<150": lambda n: n < 150, "n>=400": lambda n: n >= 400}


class Parts:
    """Seconds inside named methods of an object, per iteration (wrapped in place)."""

    def __init__(self):
        self.now = {}

    def wrap(self, obj, name, part, opens=False, closes=False):
        fn = getattr(obj, name)

        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                t1 = time.perf_counter()
                if opens:                                            # a _begin: the clock runs on until its _end returns
                    self._open = t0
                elif closes:
                    self.now[part] = self.now.get(part, 0.0) + t1 - self._open
                else:
                    self.now[part] = self.now.get(part, 0.0) + t1 - t0
        setattr(obj, name, timed)

    def take(self):
        out, self.now = self.now, {}
        return out


def single_run(q):
    from Algorithms import PCA_BO
    opt = PCA_BO(budget=BUDGET, n_DoE=NDOE, random_seed=1000 * FID + 10 * DIM, q=q)
    problem, parts, rows = BBOBProblem(FID, 0, DIM), Parts(), []
    try:
        opt._start(problem)
        ctx = opt.device_context
        for name, part in (("optimize_acqf", "optimiser"), ("gp_extend", "extend"), ("gp_truncate", "extend"),
                           ("gp_posterior", "posterior"), ("acq_eval", "scoring"), ("gp_wait_eval", "scoring")):
            parts.wrap(ctx, name, part)
        t_run = time.perf_counter()
        while opt.number_of_function_evaluations < BUDGET:
            n = len(opt.f_evals)
            t0 = time.perf_counter()
            opt._bo_iteration(problem)
            rows.append((n, time.perf_counter() - t0, parts.take()))
        seconds = time.perf_counter() - t_run
    finally:
        opt._finish()
    return rows, (BUDGET - NDOE) / seconds


def batch_run(q, B):
    from pcabo.batchrun import BatchedPCABO
    r = BatchedPCABO([BBOBProblem(FID, i, DIM) for i in range(B)], [1000 * FID + 10 * DIM + i for i in range(B)], BUDGET, NDOE,
                     acq_kernel="device", q=q)
    parts, rows = Parts(), []
    try:
        r.start()
        bt = r._batch
        for name, part, kw in (("optimize_begin", "optimiser", {"opens": True}), ("optimize_end", "optimiser", {"closes": True}),
                               ("optimize_acqf", "optimiser", {}), ("gp_extend", "extend", {}), ("gp_truncate", "extend", {}),
                               ("gp_posterior", "posterior", {}), ("acq_score_begin", "scoring", {"opens": True}),
                               ("acq_score_end", "scoring", {"closes": True}), ("gp_eval_begin", "scoring", {"opens": True}),
                               ("gp_eval_end", "scoring", {"closes": True})):
            parts.wrap(bt, name, part, **kw)
        t_run = time.perf_counter()
        while r.n < r.budget:
            n = r.n
            t0 = time.perf_counter()
            r.iteration()
            rows.append((n, time.perf_counter() - t0, parts.take()))
        seconds = time.perf_counter() - t_run
        done = sum(len(f) - NDOE for f in r.f_evals)
        parked = sum(f is not None for f in r.failed)
    finally:
        r.finish()
    return rows, done / seconds, parked


def summarise(rows):
    out = {}
    for window, inside in WINDOWS.items():
        mine = [row for row in rows if inside(row[0])]
        if not mine:
            continue
        keys = sorted({k for row in mine for k in row[2]})
        out[window] = {"iterations": len(mine), "ms_iteration": 1e3 * statistics.median(row[1] for row in mine),
                       **{"ms_" + k: 1e3 * statistics.median(row[2].get(k, 0.0) for row in mine) for k in keys}}
    return out


def over_rounds(results):
    """Median over the rounds of every figure, with the smallest and the largest round."""
    def fold(values):
        if isinstance(values[0], dict):
            return {k: fold([v[k] for v in values if k in v]) for k in values[0]}
        return {"median": statistics.median(values), "lo": min(values), "hi": max(values)}
    return fold(results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--no-single", action="store_true")
    ap.add_argument("--no-batch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("needs a HIP device")
    warnings.simplefilter("ignore", RuntimeWarning)
    out = {"library": N.lib_path(), "rounds": a.rounds, "shape": {"function": FID, "dimension": DIM, "budget": BUDGET, "n_DoE": NDOE},
           "single": {}, "batch": {}}
    if not a.no_single:
        single_run(1)                                                # warm-up: code objects, the allocator, torch
        got = {q: [] for q in a.q}
        for _ in range(a.rounds):
            for q in a.q:                                            # the q values in turn
                rows, rate = single_run(q)
                got[q].append({**summarise(rows), "evaluations_per_s": rate})
                print("single q=%d: %.1f evaluations/s" % (q, rate), file=sys.stderr, flush=True)
        out["single"] = {str(q): over_rounds(got[q]) for q in a.q}
    if not a.no_batch:
        batch_run(1, a.batch)
        got = {q: [] for q in a.q}
        for _ in range(max(1, a.rounds - 1)):
            for q in a.q:
                rows, rate, parked = batch_run(q, a.batch)
                got[q].append({**summarise(rows), "evaluations_per_s": rate, "parked_runs": parked})
                print("batch q=%d: %.1f evaluations/s" % (q, rate), file=sys.stderr, flush=True)
        out["batch"] = {"runs": a.batch, "acq_kernel": "device", **{str(q): over_rounds(got[q]) for q in a.q}}
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
