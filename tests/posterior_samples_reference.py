"""What pcabo_gp_posterior_sample / pcabo_batch_gp_posterior_sample are checked against: joint draws of the oracle's exact GP from
given base samples, in numpy longdouble - none of the library's code.

    mean, cov = posterior_reference.posterior(gp, X, noise)          (float64, the oracle's)
    A_j = cov + j s_y^2 I, j the first of 0, 1e-8, 1e-7, 1e-6 whose unblocked Cholesky meets no pivot <= 0     (longdouble)
    samples = mean + base Lc^T                                        Lc = chol(A_j), lower

MultivariateNormal.rsample(base_samples=...) behind botorch's GPyTorchPosterior, restated: BoTorch / GPyTorch are not installed here,
so parity with them is not pinned (DESIGN.md "GP posterior samples").  The ladder is psd_safe_cholesky's for float64.

SHAPES, state(), plain_queries() and nasty_queries() are the inputs of tests/test_gpu_posterior_samples.py; the CPU test
(tests/test_posterior_samples_cpu.py) shows that the forward inputs - plain queries, observation noise on - have cond_2(A) <= 1e6.
"""
import numpy as np

from ard_reference import ard_state
from posterior_reference import posterior

RUNGS = (0.0, 1e-8, 1e-7, 1e-6)
LD = np.longdouble

# (n, k, q, S, kernel, observation noise, user-supplied Normalize bounds): one block with 63 identity rows; a partial tile; an exact
# tile; a second block that is almost all padding with S across a tile; three blocks - a tile strictly below the diagonal that
# accumulates over two column blocks - with partial last tiles in q and S
SHAPES = [(9, 1, 1, 1, "matern52", False, False), (65, 3, 63, 3, "matern52", False, False), (64, 3, 64, 64, "rbf", True, False),
          (130, 9, 65, 65, "matern52", False, False), (257, 8, 130, 130, "matern52", True, True)]
KERNEL = {"matern52": 0, "rbf": 1}


def state(shape):
    """(Z, y, norm_bounds or None) of a row of SHAPES, as tests/test_gpu_posterior.py builds its states."""
    n, k, user = shape[0], shape[1], shape[6]
    Z, y = ard_state(500 + n + k, n, k)
    return Z, y, (np.vstack([Z.min(0) - 0.25, Z.max(0) + 0.5]) if user else None)


def plain_queries(Z, q, seed):
    """q points around the data, none of them near another or near a training point by construction."""
    rng = np.random.default_rng(seed)
    lo, hi = Z.min(0), Z.max(0)
    return rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), size=(q, Z.shape[1]))


def nasty_queries(Z, q, seed):
    """The same with, where there is room, two points 1e-9 apart, one training point and one exact duplicate row."""
    X = plain_queries(Z, q, seed)
    if q >= 4:
        X[1] = X[0] + 1e-9
        X[2] = Z[0]
        X[q - 1] = X[3]
    return X


def base_samples(q, S):
    """The Gaussian base of a (q, S) case: seed q + S."""
    return np.random.default_rng(q + S).standard_normal((S, q))


def cholesky_ld(A):
    """Unblocked lower Cholesky in longdouble; None when a pivot is not positive (NaN included)."""
    A = np.array(A, dtype=LD)
    q = A.shape[0]
    L = np.zeros((q, q), dtype=LD)
    for j in range(q):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < q:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def factor(cov, y_std):
    """(Lc in longdouble, the rung used, A_j in longdouble) of the ladder on cov; (None, None, None) when every rung fails."""
    cov = np.asarray(cov, dtype=LD)
    for j in RUNGS:
        A = cov + LD(j) * LD(y_std) * LD(y_std) * np.eye(cov.shape[0], dtype=LD)
        L = cholesky_ld(A)
        if L is not None:
            return L, j, A
    return None, None, None


def posterior_samples(gp, X, base, observation_noise=False, centred=False) -> dict:
    """samples (S, q) and factor (q, q) in longdouble; mean (q,), jitter, y_std, cond = cond_2(A_j) (float64 SVD)."""
    r = posterior(gp, X, observation_noise)
    L, j, A = factor(r["covariance"], r["y_std"])
    if L is None:
        raise np.linalg.LinAlgError("no rung of the ladder could be factored")
    draws = np.asarray(base, dtype=LD) @ L.T
    if not centred:
        draws = draws + np.asarray(r["mean"], dtype=LD)
    return {"samples": draws, "mean": r["mean"], "jitter": j, "factor": L, "y_std": r["y_std"],
            "cond": float(np.linalg.cond(np.asarray(A, dtype=np.float64))), "covariance": r["covariance"]}
