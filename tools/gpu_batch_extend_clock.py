"""Cost of appending points to the GPs of a lock-step batch (Batch.gp_extend) and of taking them back (Batch.gp_truncate), next to
the same calls made on B single contexts one after the other, on the same device in the same process.  The protocol of
gpu_extend_clock.py: device-synchronised host clocks (every call returns after a wait on its stream), --reps calls after a warm-up,
the two routes timed in turn --rounds times, the median of the rounds' medians with their spread.

A state can only be extended so often, so what is timed is the PAIR extend + truncate: one point, eight points.  Before the clock
starts the two routes are compared: every run of the batch must hold the bytes of its single context after the extend.

usage: gpu_batch_extend_clock.py [--runs 30] [--shape 450x36] [--reps 100] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.environ.get("PCABO_TREE", ROOT), "para-ortho-pca-bo_amd"))
from gpu_extend_clock import rounds, state                          # noqa: E402
from pcabo import _native as N                                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--shape", default="450x36")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("needs a HIP device")
    B = a.runs
    n, k = (int(v) for v in a.shape.split("x"))
    Z, y = (np.stack(v) for v in zip(*[state(1000 * b + n + k, n + 8, k) for b in range(B)]))
    bt = N.Batch(B, max_n=n + 8, max_d=k, max_q=64)
    bt.gp_condition_begin(np.ascontiguousarray(Z[:, :n]), np.ascontiguousarray(y[:, :n]))
    _, status = bt.gp_wait_eval([Z[b, :4] for b in range(B)], y[:, :n].min(axis=1))
    assert not status.any()
    singles = [N.Context(max_n=n + 8, max_d=k, max_q=64) for _ in range(B)]
    for b, c in enumerate(singles):
        c.gp_condition(y[b, :n], Z=Z[b, :n])
    new = {p: ([np.ascontiguousarray(Z[b, n:n + p]) for b in range(B)], np.ascontiguousarray(y[:, n:n + p])) for p in (1, 8)}

    # the two routes give the same bytes
    for p in (1, 8):
        _, status = bt.gp_extend(*new[p])
        assert not status.any()
        for b, c in enumerate(singles):
            c.gp_extend(new[p][0][b], new[p][1][b])
            one, two = c.gp_state(), bt.ctx[b].gp_state()
            assert all(one[key].tobytes() == two[key].tobytes() for key in ("L", "R", "alpha")), (p, b)
            c.gp_truncate()
        bt.gp_truncate()

    def batch_pair(p):
        bt.gp_extend(*new[p])
        bt.gp_truncate()

    def singles_pair(p):
        for b, c in enumerate(singles):
            c.gp_extend(new[p][0][b], new[p][1][b])
            c.gp_truncate()

    res = rounds([("batch_extend1+truncate", lambda: batch_pair(1)), ("singles_extend1+truncate", lambda: singles_pair(1)),
                  ("batch_extend8+truncate", lambda: batch_pair(8)), ("singles_extend8+truncate", lambda: singles_pair(8))],
                 a.reps, a.rounds)
    row = {"what": "batch against singles", "runs": B, "n": n, "k": k, **res}
    for p in (1, 8):
        row["singles_over_batch_%d" % p] = res["singles_extend%d+truncate" % p]["ms_median"] / res["batch_extend%d+truncate" % p]["ms_median"]
    print(json.dumps(row))
    print(json.dumps({"library": N.lib_path(), "reps": a.reps, "rounds": a.rounds}))
    for c in singles:
        c.close()
    bt.close()


if __name__ == "__main__":
    main()
