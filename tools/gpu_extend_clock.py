"""Cost of appending points to a conditioned GP (Context.gp_extend) and of taking them back (gp_truncate), next to
the only other route to the same number of points: a fresh gp_condition on n + p points (which is not even the same model - it
refits Normalize and Standardize).  Device-synchronised host clocks (every call returns after a wait on the stream), medians and
minima over --reps calls after a warm-up; the routes are timed in turn on the same state, --rounds times, and the median of the
rounds' medians is reported with their spread (the method of gpu_loo_clock.py).

A state can only be extended so often, so the routes timed in turn are the PAIRS extend + truncate (one point, eight points, eight
points in believer mode) and the conditionings; behind them the parts are timed on their own - extend of one and of eight points,
truncate of eight - each call bracketed by the other half of its pair outside the clock.  Rows: a single context at each --shape
(n x k).  The model of the traffic is printed beside the times: per point four passes over the lower triangle of R (v = R ks and
w = R^T v read it once each, alpha = R^T (R y_s) once each again when it follows the point), 16 n^2 bytes.  No threshold.

usage: gpu_extend_clock.py [--shape 450x36 --shape 1050x89] [--reps 100] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.environ.get("PCABO_TREE", ROOT), "para-ortho-pca-bo_amd"))
from pcabo import _native as N                                      # noqa: E402


def clock(fn, reps):
    for _ in range(10):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def state(seed, n, k):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-2.0, 2.0, size=(n, k))
    return Z, np.sin(3.0 * Z[:, 0]) + 0.5 * (Z ** 2).sum(1) + 0.1 * rng.standard_normal(n)


def rounds(pairs, reps, nrounds):
    """{name: (median of the rounds' medians, smallest and largest of them, smallest single call)}, the routes timed in turn."""
    meds, mins = {name: [] for name, _ in pairs}, {name: [] for name, _ in pairs}
    for _ in range(nrounds):
        for name, fn in pairs:
            med, lo = clock(fn, reps)
            meds[name].append(med)
            mins[name].append(lo)
    return {name: {"ms_median": statistics.median(meds[name]), "ms_median_lo": min(meds[name]), "ms_median_hi": max(meds[name]),
                   "ms_min": min(mins[name])} for name, _ in pairs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("needs a HIP device")
    shapes = [tuple(int(v) for v in s.split("x")) for s in (a.shape or ["450x36", "1050x89"])]
    out = {"library": N.lib_path(), "reps": a.reps, "rounds": a.rounds, "rows": []}
    for n, k in shapes:
        Z, y = state(n + k, n + 8, k)
        ctx = N.Context(max_n=n + 8, max_d=k, max_q=64)
        ctx.gp_condition(y[:n], Z=Z[:n])

        def pair(p):
            ctx.gp_extend(Z[n:n + p], y[n:n + p])
            ctx.gp_truncate()

        res = rounds([("extend1+truncate", lambda: pair(1)), ("extend8+truncate", lambda: pair(8)),
                      ("believer8+truncate", lambda: (ctx.gp_extend(Z[n:n + 8]), ctx.gp_truncate())),
                      ("condition_n+1", lambda: ctx.gp_condition(y[:n + 1], Z=Z[:n + 1])),
                      ("condition_n+8", lambda: ctx.gp_condition(y[:n + 8], Z=Z[:n + 8])),
                      ("condition_n", lambda: ctx.gp_condition(y[:n], Z=Z[:n]))], a.reps, a.rounds)
        # the parts on their own: the other half of the pair runs outside the clock
        ts = []
        for _ in range(a.reps):
            ctx.gp_extend(Z[n:n + 8], y[n:n + 8])
            t0 = time.perf_counter()
            ctx.gp_truncate()
            ts.append((time.perf_counter() - t0) * 1e3)
        res["truncate8"] = {"ms_median": statistics.median(ts), "ms_min": min(ts)}
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.gp_extend(Z[n:n + 1], y[n:n + 1])
            ts.append((time.perf_counter() - t0) * 1e3)
            ctx.gp_truncate()
        res["extend1"] = {"ms_median": statistics.median(ts), "ms_min": min(ts)}
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.gp_extend(Z[n:n + 8], y[n:n + 8])
            ts.append((time.perf_counter() - t0) * 1e3)
            ctx.gp_truncate()
        res["extend8"] = {"ms_median": statistics.median(ts), "ms_min": min(ts)}
        out["rows"].append({"what": "context", "n": n, "k": k, "bytes_per_point_model": 16 * n * n, **res})
        ctx.close()
    for row in out["rows"]:
        print(json.dumps(row))
    print(json.dumps({key: out[key] for key in ("library", "reps", "rounds")}))


if __name__ == "__main__":
    main()
