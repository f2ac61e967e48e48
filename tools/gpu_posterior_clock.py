"""Cost of a posterior query (Context.gp_posterior) next to the value-only scoring of the same points (Context.acq_eval, grad=False):
device-synchronised host clocks (every call returns after a wait on the stream), medians over --reps calls after a warm-up.

Prints ms per call of the scoring, of a mean + variance query and of a query with the covariance, and the work of k_post_cov:
2 NP q^2 / 2 FLOP in the model (the lower half of V^T V), what its whole 64 x 64 tiles issue on the MFMAs, and the time both take at
the FP64 MFMA peak.  k_post_cov's own time comes from a separate run under `rocprofv3 --kernel-trace --stats`.  With --scoring-only
only the scoring is timed (a library without the posterior entry points, for the comparison with an earlier build).

A sampling row follows the covariance query of the same q: ms per call of Context.gp_posterior_samples with --samples base samples
(observation noise on, so the first rung factors), and the work of k_post_sample in the same three forms.  No threshold.

usage: gpu_posterior_clock.py [--shape 449x36] [--q 512] [--samples 256] [--reps 200] [--scoring-only]"""
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

FP64_PEAK = 78.6e12                                                  # FP64 MFMA, MI355X


def clock(fn, reps):
    for _ in range(10):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="449x36")
    ap.add_argument("--q", type=int, default=512)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--scoring-only", action="store_true")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("needs a HIP device")
    n, k = (int(v) for v in a.shape.split("x"))
    rng = np.random.default_rng(0)
    Z = rng.uniform(-2.0, 2.0, size=(n, k))
    y = np.sin(3.0 * Z[:, 0]) + 0.5 * (Z ** 2).sum(1) + 0.1 * rng.standard_normal(n)
    X = rng.uniform(-2.0, 2.0, size=(a.q, k))
    ctx = N.Context(max_n=n, max_d=k, max_q=a.q)
    ctx.gp_condition(y, Z=Z)
    row = {"n": n, "k": k, "q": a.q, "reps": a.reps, "library": N.lib_path()}
    row["ms_scoring_median"], row["ms_scoring_min"] = clock(lambda: ctx.acq_eval(X, 0.0, True, N.ACQ_UCB, grad=False), a.reps)
    if not a.scoring_only:
        row["ms_mean_var_median"], row["ms_mean_var_min"] = clock(lambda: ctx.gp_posterior(X), a.reps)
        row["ms_cov_median"], row["ms_cov_min"] = clock(lambda: ctx.gp_posterior(X, covariance=True), a.reps)
        NP, nt = -(-n // 64) * 64, -(-a.q // 64)
        row["cov_model_flops"] = 2.0 * NP * a.q * a.q / 2.0
        row["cov_issued_flops"] = 2.0 * 64 * 64 * NP * (nt * (nt + 1) // 2)
        row["cov_issued_us_at_peak"] = row["cov_issued_flops"] / FP64_PEAK * 1e6
        row["ms_cov_noisy_median"], row["ms_cov_noisy_min"] = clock(
            lambda: ctx.gp_posterior(X, observation_noise=True, covariance=True), a.reps)
        base = np.random.default_rng(1).standard_normal((a.samples, a.q))
        draw = lambda: ctx.gp_posterior_samples(X, base_samples=base, observation_noise=True)      # noqa: E731
        row["samples"], row["sample_jitter"] = a.samples, draw()["jitter"]
        row["ms_sample_median"], row["ms_sample_min"] = clock(draw, a.reps)
        row["sample_model_flops"] = 2.0 * a.samples * a.q * a.q / 2.0
        row["sample_issued_flops"] = 2.0 * 64 * 64 * 64 * -(-a.samples // 64) * (nt * (nt + 1) // 2)
        row["sample_issued_us_at_peak"] = row["sample_issued_flops"] / FP64_PEAK * 1e6
    ctx.close()
    print(json.dumps(row))


if __name__ == "__main__":
    main()
