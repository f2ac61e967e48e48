"""The upper confidence bound on the oracle's exact GP, and the states the UCB tests share.

No tests here: `test_ucb_cpu.py` drives the host optimiser over this surface, `test_gpu_ucb.py` judges the HIP kernels
(`acq_scalar_chain` in acq_math.h, called from kernels_acq.hip and kernels_lbfgsb.hip) and whole runs by it.

botorch's `UpperConfidenceBound` as published (botorch/acquisition/analytic.py):

    mean, sigma = self._mean_and_sigma(X)                       # sigma = var.clamp_min(1e-12).sqrt()
    return (mean if self.maximize else -mean) + self.beta.sqrt() * sigma

with `beta` registered as `torch.as_tensor(beta)`: float32 for a Python float, so `beta.sqrt()` is a float32 root that type
promotion then carries into the float64 product unchanged.  botorch is not installed and the reference never evaluates UCB
(it fails while constructing it), so nothing pins this restatement against a run of botorch: parity unpinned.
"""
import numpy as np
import torch

import pcabo_oracle as O
from pcabo.bbob import BBOBProblem


def kappa_of(beta) -> float:
    return float(torch.as_tensor(float(beta)).sqrt())


class UCBReference(O.Acquisition):
    """`O.Acquisition` with the UCB formula: `value_and_grad`, `O.gen_candidates_scipy`, `O.gen_batch_initial_conditions` and
    `O.optimize_acqf` work with it unchanged (any `kind` but PI takes `initialize_q_batch`)."""

    def __init__(self, gp: O.ExactGP, beta: float, maximize: bool):
        self.gp, self.maximize, self.kind = gp, bool(maximize), "upper_confidence_bound"
        self.beta, self.kappa, self.best_f = float(beta), kappa_of(beta), None

    def __call__(self, X: torch.Tensor) -> torch.Tensor:
        mean, var = self.gp.posterior(X)
        sigma = var.clamp_min(O.ACQ_MIN_VAR).sqrt()
        return (mean if self.maximize else -mean) + self.kappa * sigma


# (fid, d, n, beta, maximize): the surfaces of test_ucb_cpu.py's comparison with scipy
CPU_STATES = ((15, 4, 9, 2.0, False), (15, 6, 17, 0.25, False), (17, 10, 70, 4.0, True), (15, 10, 130, 2.0, False),
              (16, 20, 61, 2.0, False), (15, 6, 30, 9.0, False))


def bbob_state(fid, d, n, beta, maximize):
    """n uniform points of [-5, 5]^d on BBOBProblem(fid, 1, d), all from default_rng(n), through the oracle's wPCA and GP.
    Returns (reference UCB, 2 x k search box)."""
    rng = np.random.default_rng(n)
    X = rng.uniform(-5.0, 5.0, size=(n, d))
    prob = BBOBProblem(fid, 1, d)
    f = np.array([prob(x) for x in X], dtype=np.float64)
    wp = O.weighted_pca(X, f, maximize, 0.95, 0, noise=rng.normal(0, 1e-8, size=X.shape))
    gp = O.ExactGP(wp.Z, f, O.normalize_bounds(wp.Z))
    return UCBReference(gp, beta, maximize), O.acq_bounds(wp.Z)
