"""Cost of the lock-step GP hyperparameter fit of a batch (Batch.gp_fit) against the same fits one after the other
(Context.gp_fit on stand-alone contexts) - device-synchronised host clocks: every call below returns after a wait on the stream.

B seeded states (those of tools/gpu_gp_fit_clock.py, seed = run) of n points in d dimensions, conditioned through
Batch.gp_condition_begin (bounds from the data).  Prints: ms per lock-step fit (the conditioning call that stages the inputs
included), its rounds (launch sequences), the sum of the runs' evaluations, the wasted share 1 - sum nfev_b / (B * rounds) - run
slots of the launches spent on runs that had finished (their final evaluation counted as work) - and, as the yardstick, ms for
the same B fits done one after the other.  Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats`.

--ard: the fit with one lengthscale per input (Batch.gp_fit_ard against Context.gp_fit_ard).

usage: gpu_batch_fit_clock.py B n d [--reps 3] [--ard]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pcabo import _native as N                                      # noqa: E402
from gpu_gp_fit_clock import seeded_state                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("B", type=int)
    ap.add_argument("n", type=int)
    ap.add_argument("d", type=int)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ard", action="store_true", help="one lengthscale per input: Batch.gp_fit_ard against Context.gp_fit_ard")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("needs a HIP device")
    B, n, d = a.B, a.n, a.d
    states = [seeded_state(n, d, seed=b) for b in range(B)]
    Z, y = np.stack([s[0] for s in states]), np.stack([s[1] for s in states])
    bt = N.Batch(B, max_n=n, max_d=d, max_q=64)

    def lockstep():
        bt.gp_condition_begin(Z, y)
        return bt.gp_fit_ard() if a.ard else bt.gp_fit()

    def clocked(call):
        """(last result, ms of every repetition) after one warm-up call"""
        out, ms = call(), []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return out, ms
    fits, lock_reps = clocked(lockstep)
    lock_ms = float(np.mean(lock_reps))
    rounds = bt.fit_rounds
    bt.close()
    nfev = [f["evaluations"] for f in fits]
    ctxs = [N.Context(max_n=n, max_d=d, max_q=64) for _ in range(min(B, 4))]       # (a context per run would only cost memory)

    def sequential():
        return [(ctxs[b % len(ctxs)].gp_fit_ard if a.ard else ctxs[b % len(ctxs)].gp_fit)(y[b], Z=Z[b]) for b in range(B)]
    one, seq_reps = clocked(sequential)
    seq_ms = float(np.mean(seq_reps))
    for c in ctxs:
        c.close()
    same = all(f["theta"].tobytes() == o["theta"].tobytes() and f["evaluations"] == o["evaluations"] for f, o in zip(fits, one))
    row = {"B": B, "n": n, "d": d, "ard": bool(a.ard), "ms_lockstep_fit": lock_ms, "ms_lockstep_reps": lock_reps,
           "ms_sequential_reps": seq_reps, "ms_per_round": lock_ms / rounds, "rounds": rounds, "sum_nfev": int(sum(nfev)),
           "min_nfev": int(min(nfev)), "max_nfev": int(max(nfev)), "wasted_share": 1.0 - sum(nfev) / (B * rounds),
           "ms_sequential_fits": seq_ms, "sequential_over_lockstep": seq_ms / lock_ms, "bit_identical": bool(same),
           "warnflags": sorted({f["warnflag"] for f in fits})}
    print(f"B={B} n={n} d={d}{' ARD' if a.ard else ''}: lock-step fit {lock_ms:8.2f} ms, {rounds} rounds, sum nfev {row['sum_nfev']} "
          f"(min {row['min_nfev']}, max {row['max_nfev']}), wasted share {100 * row['wasted_share']:.1f} %, bit-identical to the "
          f"single fits: {same}", flush=True)
    print(f"the same {B} fits one after the other (Context.{'gp_fit_ard' if a.ard else 'gp_fit'}): {seq_ms:8.2f} ms = {row['sequential_over_lockstep']:.2f} x "
          "the lock-step fit", flush=True)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
