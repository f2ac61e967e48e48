#!/usr/bin/env python3
"""Host clock of pcabo._native.pack_rows against the loops that stood inline in Batch before it (CPU only, no device):

    python tools/cpu_pack_clock.py [OUT.json]

Two shapes: B = 30 runs of q = 512 points, k = 36 of max_d = 40, drawn in place in the kept row buffer (the no-copy case of every
lock-step iteration: gp_eval_begin), and B = 60 single points of k = 36 into a fresh buffer (the inverse map).  Five repetitions,
each the median of 1 000 calls of either, the two alternating call by call in one process.  Microseconds per call."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))
from pcabo._native import pack_rows  # noqa: E402


def inline_reuse(blocks, B, row, buf):          # gp_eval_begin as it stood
    for b, xq in enumerate(blocks):
        if not (isinstance(xq, np.ndarray) and xq.base is buf):
            buf[b, : xq.size] = np.ascontiguousarray(xq, dtype=np.float64).ravel()
    return buf


def inline_fresh(blocks, B, row, buf):          # _pack_z as it stood
    z = np.zeros((B, row))
    for b, zb in enumerate(blocks):
        z[b, : zb.size] = np.asarray(zb, dtype=np.float64).ravel()
    return z


def new_reuse(blocks, B, row, buf):
    return pack_rows(blocks, row, buf)


def new_fresh(blocks, B, row, buf):             # Batch._packed
    return pack_rows(blocks, row) if len(blocks) == B else pack_rows(blocks, row, np.zeros((B, row)))


def clock(old, new, blocks, B, row, buf, calls=1000, reps=5):
    meds = {"inline": [], "pack_rows": []}
    for _ in range(reps):
        t = {"inline": [], "pack_rows": []}
        for _ in range(calls):
            for name, fn in (("inline", old), ("pack_rows", new)):
                t0 = time.perf_counter()
                fn(blocks, B, row, buf)
                t[name].append(time.perf_counter() - t0)
        for name in t:
            meds[name].append(round(1e6 * statistics.median(t[name]), 3))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "repetitions_us": v} for name, v in meds.items()}


def main():
    rng = np.random.default_rng(0)
    B, q, k, md = 30, 512, 36, 40
    buf = np.zeros((B, q * md))
    views = [buf[b, : q * k].reshape(q, k) for b in range(B)]
    for v in views:
        v[:] = rng.standard_normal((q, k))
    z = [rng.standard_normal(k) for _ in range(60)]
    out = {"rows_in_place_B30_q512_k36": clock(inline_reuse, new_reuse, views, B, q * md, buf),
           "inverse_map_B60_q1_k36": clock(inline_fresh, new_fresh, z, 60, md, None)}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
