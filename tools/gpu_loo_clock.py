"""Cost of the leave-one-out predictions (Context.gp_loo, Batch.gp_loo) next to the route there was before them: the root inverse
brought to the host (pcabo_get_gp_state with Rinv, alpha and the Standardize statistics only - the least that route needs) and the
closed form in numpy, once per run.  Device-synchronised host clocks (every call returns after a wait on the stream), medians and
minima over --reps calls after a warm-up; both routes are timed in turn on the same conditioned states, --rounds times, and the
median of the rounds' medians is reported with their spread.

Rows: a single context at each --shape (n x k), and a batch of --runs runs at the first shape (Batch.gp_loo: one launch and one
strided copy for all runs; the other route: one single-context call and one numpy pass per run).  The model of k_loo's traffic is
printed beside the times: n (n + 1) / 2 doubles of R read (whole 512-byte row segments: the 64-column blocks' triangles), 4 n
doubles written.  k_loo's own time comes from a separate run under `rocprofv3 --kernel-trace --stats`.  No threshold.

usage: gpu_loo_clock.py [--shape 450x36 --shape 1050x89] [--runs 30] [--reps 200] [--rounds 3]"""
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

LOG2PI = float(np.log(2.0 * np.pi))


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


def host_route(ctx, y):
    """The earlier route for one context: R, alpha and (m', s) to the host, the closed form in numpy."""
    n = ctx.n
    R, alpha, ms = np.empty((n, n)), np.empty(n), np.empty(2)
    ctx._chk(N.LIB.pcabo_get_gp_state(ctx._h, None, N._ptr(R), N._ptr(alpha), N._ptr(ms), None))
    R = np.tril(R)
    d = np.einsum("pi,pi->i", R, R)
    r = alpha / d
    var = ms[1] * ms[1] / d
    z = r * np.sqrt(d)
    lpd = -0.5 * (LOG2PI + np.log(var) + z * z)
    return {"mean": ms[0] + ms[1] * ((y - ms[0]) / ms[1] - r), "variance": var, "z": z, "lpd": lpd, "lpd_sum": float(lpd.sum())}


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


def traffic(n):
    nb = -(-n // 64)
    rows = sum(n - 64 * j for j in range(nb))                     # row segments of 64 doubles the column blocks read
    return {"read_doubles_model": n * (n + 1) // 2, "read_doubles_issued": 64 * rows, "written_doubles": 4 * n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("needs a HIP device")
    shapes = [tuple(int(v) for v in s.split("x")) for s in (a.shape or ["450x36", "1050x89"])]
    out = {"library": N.lib_path(), "reps": a.reps, "rounds": a.rounds, "rows": []}
    for n, k in shapes:
        Z, y = state(n + k, n, k)
        ctx = N.Context(max_n=n, max_d=k, max_q=64)
        ctx.gp_condition(y, Z=Z)
        dev, host = ctx.gp_loo(), host_route(ctx, y)
        worst = max(float(np.abs(dev[key] - host[key]).max() / np.abs(host[key]).max()) for key in ("mean", "variance", "z", "lpd"))
        res = rounds([("gp_loo", ctx.gp_loo), ("state_numpy", lambda: host_route(ctx, y))], a.reps, a.rounds)
        out["rows"].append({"what": "context", "n": n, "k": k, "agreement": worst, **traffic(n), **res})
        ctx.close()
    n, k = shapes[0]
    B = a.runs
    states = [state(1000 + b, n, k) for b in range(B)]
    Zs, ys = np.stack([s[0] for s in states]), np.stack([s[1] for s in states])
    bt = N.Batch(B, max_n=n, max_d=k, max_q=64)
    bt.gp_condition_begin(Zs, ys)
    _, status = bt.gp_wait_eval([np.zeros((64, k))] * B, ys.min(axis=1))
    assert (status == 0).all()
    assert all(r is not None for r in bt.gp_loo())
    res = rounds([("gp_loo", bt.gp_loo), ("state_numpy", lambda: [host_route(bt.ctx[b], ys[b]) for b in range(B)])],
                 max(a.reps // 4, 10), a.rounds)
    out["rows"].append({"what": "batch", "runs": B, "n": n, "k": k, **res})
    bt.close()
    for row in out["rows"]:
        print(json.dumps(row))
    print(json.dumps({key: out[key] for key in ("library", "reps", "rounds")}))


if __name__ == "__main__":
    main()
