"""One process's clocks of the GP fit's calls, for comparing two builds of the library (PCABO_LIB selects the build; run the two in
alternating processes and compare medians over the processes): Context.gp_mll and gp_mll_ard at the two shapes DESIGN.md quotes,
(450, 36) and (1050, 89), at the states of tools/gpu_gp_fit_clock.py, and one gp_fit and one gp_fit_ard at the (70, 33) state of
tests/ard_reference.py's FIT_STATES.  Device-synchronised host clocks (every call returns after a wait on the stream), each call
warmed up first; ms per call, the mean of --reps calls (fits: --fit-reps).  Prints one JSON line.

usage: gpu_fit_pair_clock.py [--reps 40] [--fit-reps 3]"""
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
from gpu_gp_fit_clock import clock, seeded_state                    # noqa: E402

FIT_SEED, FIT_N, FIT_K = 4, 70, 33                                   # tests/ard_reference.py: FIT_STATES[2] and its ard_state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--fit-reps", type=int, default=3)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("needs a HIP device")
    out = {"lib": os.environ.get("PCABO_LIB", "")}
    for n, k in ((450, 36), (1050, 89)):
        Z, y = seeded_state(n, k)
        ctx = N.Context(max_n=n, max_d=k, max_q=64)
        th = np.r_[0.05, 0.3, np.random.default_rng(k).uniform(-0.5, 1.0, size=k)]
        out["gp_mll_%dx%d" % (n, k)] = clock(lambda: ctx.gp_mll(y, th[:3], Z=Z), a.reps)
        out["gp_mll_ard_%dx%d" % (n, k)] = clock(lambda: ctx.gp_mll_ard(y, th, Z=Z), a.reps)
        ctx.close()
    rng = np.random.default_rng(FIT_SEED)                            # ard_state(4, 70, 33)
    Z = rng.uniform(-2.0, 2.0, size=(FIT_N, FIT_K))
    y = np.sin(3.0 * Z[:, 0]) + 0.5 * (Z[:, :2] ** 2).sum(1) + 0.1 * rng.standard_normal(FIT_N)
    ctx = N.Context(max_n=FIT_N, max_d=FIT_K, max_q=64)
    out["gp_fit_%dx%d" % (FIT_N, FIT_K)] = clock(lambda: ctx.gp_fit(y, Z=Z), a.fit_reps)
    out["gp_fit_ard_%dx%d" % (FIT_N, FIT_K)] = clock(lambda: ctx.gp_fit_ard(y, Z=Z), a.fit_reps)
    out["evaluations"] = [ctx.gp_fit(y, Z=Z)["evaluations"], ctx.gp_fit_ard(y, Z=Z)["evaluations"]]
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
