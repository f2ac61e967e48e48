"""What pcabo_gp_posterior / pcabo_batch_gp_posterior are checked against: posterior mean, variance and joint covariance of the
oracle's exact GP, from its public members only (ExactGP.alpha, .Linv, .lo, .coef, .Zn, .y_mean, .y_std and kernel_matrix) - none of
the library's code.

    mean = y_mean + y_std ks alpha                               ks = k(Xn, Zn)
    cov  = y_std^2 (k(Xn, Xn) [+ s2 I] - V^T V)                  V = Linv ks^T, not floored
    variance = diag(cov) floored at 1e-10 (gpytorch's min_variance in float64)

gpytorch's semantics for SingleTaskGP(MaternKernel | RBFKernel, Standardize, Normalize) without an output scale, restated: BoTorch /
GPyTorch are not installed here, so parity with them is not pinned (DESIGN.md "GP posterior queries").  Fitted states: the GP comes
from ard_reference.fitted_gp (a scalar fit is the ARD model with equal lengthscales; scalar_fit_as_ard below).
"""
import numpy as np
import torch

import pcabo_oracle as O

MIN_VARIANCE = 1e-10


def posterior(gp: "O.ExactGP", X, observation_noise: bool = False) -> dict:
    """mean (q,), variance (q,), covariance (q, q) and raw_variance (q,) = diag(covariance), the variance before the floor."""
    gp.condition()
    X = torch.as_tensor(np.asarray(X, dtype=np.float64)).reshape(-1, gp.k)
    Xn = (X - gp.lo) / gp.coef
    ks = O.kernel_matrix(Xn, gp.Zn, gp.lengthscale, gp.kernel)            # q x n
    V = gp.Linv @ ks.mT                                                   # n x q
    prior = O.kernel_matrix(Xn, Xn, gp.lengthscale, gp.kernel)            # q x q, unit diagonal
    if observation_noise:
        prior = prior + float(gp.noise) * torch.eye(X.shape[0], dtype=torch.float64)
    sy = gp.y_std.view(())
    cov = (prior - V.mT @ V) * sy ** 2
    raw = torch.diagonal(cov).clone()
    return {"mean": (gp.y_mean.view(()) + sy * (ks @ gp.alpha)).numpy(), "variance": raw.clamp_min(MIN_VARIANCE).numpy(),
            "covariance": cov.numpy(), "raw_variance": raw.numpy(), "y_std": float(sy)}


def scalar_fit_as_ard(hp: dict, k: int) -> dict:
    """The dict of a scalar fit (Context.gp_fit) in the form ard_reference.fitted_gp reads: k equal lengthscales."""
    return {"lengthscales": np.full(k, hp["lengthscale"]), "noise": hp["noise"], "mean_constant": hp["mean_constant"]}


def conditioned_on_one_more(gp: "O.ExactGP", Z, x) -> "O.ExactGP":
    """The oracle GP on the n + 1 points (Z, x) with gp's Normalize bounds, hyperparameters and Standardize statistics held fixed
    (the value observed at x does not enter a variance)."""
    Z1 = np.vstack([np.asarray(Z, dtype=np.float64), np.asarray(x, dtype=np.float64).reshape(1, -1)])
    g1 = O.ExactGP(Z1, np.zeros(Z1.shape[0]), gp.norm_bounds, lengthscale=gp.lengthscale, noise=gp.noise, kernel=gp.kernel)
    g1.y_mean, g1.y_std = gp.y_mean, gp.y_std
    g1.y_s = torch.zeros(Z1.shape[0], dtype=torch.float64)
    return g1
