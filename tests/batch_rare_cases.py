"""Inputs of the rare paths of a lock-step batch: one run of it needs the jitter ladder, or ends without a GP, beside runs that do
neither.  No tests here: `test_batch_rare_cases_cpu.py` proves on the CPU what every input is there for (which rung the numpy
restatement of the conditioning needs, or that none works, with margins), `test_gpu_batch_rare_paths.py` drives the batches.

All inputs have n = 130 points (three 64-row tiles' worth of rows: NP = 192), the Matern-5/2 kernel at the default lengthscale and
noise 0 - with noise the ladder is never needed.
  retry   `retry_case()` of test_gpu_score_split.py (imported, not copied): k = 3, two points copied seven times each on both sides
          of the 64-row boundary.  K is singular up to rounding; rung 0 fails, 1e-8 is decisively positive definite.
  plain   seeded uniform points, k = 3: factored at rung 0 with a smallest pivot >= 1e3 n eps ||K||, so "rung 0 goes either way"
          cannot apply to them.
  dead    a plain case with one column constant and no Normalize bounds: the range is 0, the distance NaN, every rung fails.
  tail    the first 64 rows of `retry` (three extra copies of two points each) and 66 plain rows behind them.
  wPCA    X in d = 6 whose leading k_b columns carry the spread (the others 1e-4 of it), k_b = 5, 3, 4 at var_threshold 0.999; the
          middle run's X has the duplicate-row pattern of `retry`, so its projected points have exact duplicates.
"""
from types import SimpleNamespace

import numpy as np

import gp_reference as G
from test_gpu_score_split import retry_case

N, K, D = 130, 3, 6
EPS = 2.0 ** -52
MARGIN = 1e3                                                       # smallest pivot / (n eps ||K||_2), as test_gp_reference_cpu.py asks
DUP_A = (5, 20, 37, 66, 81, 99, 127)                               # rows that copy row 2 in retry_case()
DUP_B = (9, 30, 63, 64, 70, 111, 128)                              # ... and row 3
WPCA_K = (5, 3, 4)
VAR_THRESHOLD = 0.999
DEAD_COLUMN = 1


def as_case(Z, y, name):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    return SimpleNamespace(id=name, gen="lhs", hyper="default", Z=Z, y=np.ascontiguousarray(y, dtype=np.float64), n=Z.shape[0],
                           k=Z.shape[1], lengthscale=G.LENGTHSCALE, noise=0.0, kernel="matern", norm_bounds=None)


def retry():
    Z, y, _ = retry_case()
    return as_case(Z, y, "retry")


def plain(seed, k=K):
    """Run `seed`'s own well-separated points."""
    rng = np.random.default_rng([1308, seed, k])
    return as_case(rng.uniform(-1.0, 1.0, (N, k)), rng.normal(size=N) * 200.0 + 900.0, "plain%d" % seed)


def dead(seed):
    c = plain(seed)
    c.Z[:, DEAD_COLUMN] = 0.25
    c.id = "dead%d" % seed
    return c


def retry_tail():
    """64 + 66 rows: what the jitter redo meets when the singular part lies in the first tile alone."""
    c = retry()
    c.Z[64:] = plain(77).Z[:N - 64]
    c.id = "retry-tail"
    return c


def probes(case, q, seed=0):
    lo, hi = case.Z.min(axis=0), case.Z.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    return np.random.default_rng([seed, q, case.k, 17]).uniform(lo - 0.05 * span, hi + 0.05 * span, size=(q, case.k))


def new_points(case, p, seed=0):
    """p points drawn uniformly from the data's range (never a copy of a training point: at noise 0 a copy makes d2 a difference of
    rounding errors) and their values."""
    rng = np.random.default_rng([seed, p, case.k, 23])
    return rng.uniform(case.Z.min(axis=0), case.Z.max(axis=0), size=(p, case.k)), rng.normal(size=p) * 200.0 + 900.0


def best_of(case):
    return float(np.float32(np.median(case.y)))


def wpca_inputs():
    """(X[B, n, d], y[B, n], ranks[B, n], noise[B, n, d]) of the fused route; the noise is zero, so the oracle and the device see
    the same centred data."""
    X, y = np.empty((3, N, D)), np.empty((3, N))
    for b, k in enumerate(WPCA_K):
        rng = np.random.default_rng([9100, b])
        Z = rng.uniform(-1.0, 1.0, (N, k))
        X[b] = 1e-4 * rng.uniform(-2.0, 2.0, (N, D))
        X[b, :, :k] = Z
        y[b] = rng.normal(size=N) * 200.0 + 900.0
    X[1, DUP_A, :] = X[1, 2]
    X[1, DUP_B, :] = X[1, 3]
    ranks = np.argsort(np.argsort(y, axis=1), axis=1).astype(np.int64) + 1
    return X, y, ranks, np.zeros_like(X)


def pivot_margin(case, jitter=0.0):
    """Smallest pivot of the restatement's factorisation of K + jitter I over n eps ||K||_2 (raises np.linalg.LinAlgError if none)."""
    res = G.restate(case, jitter=jitter)
    return float((np.diag(res.L) ** 2).min() / (case.n * EPS * np.linalg.norm(res.K, 2)))
