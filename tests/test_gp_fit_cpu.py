"""Opt-in GP hyperparameter fit (PCA_BO / Vanilla_BO fit_gp=True), host side.

The restated model: the reference's SingleTaskGP(MaternKernel(2.5), Standardize, Normalize) with its default ConstantMean and
likelihood (LogNormalPrior(-4, 1) on the noise, GreaterThan(1e-4)), fitted the way fit_gpytorch_mll(ExactMarginalLogLikelihood)
does it: scipy's L-BFGS-B with its defaults on the loss

    loss(theta) = -[log N(y_s; c 1, K_l + s2 I) + log LogNormal(s2; -4, 1)] / n,   theta = (s2, c, rho), l = softplus(rho).

BoTorch / GPyTorch are not installed here, so this restatement is not pinned against them (DESIGN.md "GP hyperparameter fit").
The device fit (tests/test_gpu_gp_fit.py) is checked against the functions below.
"""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import pcabo_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA0 = (math.exp(-5.0), 0.0, 0.0)                     # the model's initial values (noise, mean constant, raw lengthscale)
NOISE_LB = 1e-4                                          # GreaterThan(1e-4), no transform: a bound of the optimiser
LOG2PI = math.log(2.0 * math.pi)


def restated_loss(Zn: torch.Tensor, ys: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """The fit's loss, torch float64 autograd through the oracle's Matern-5/2 Gram (the psd_safe_cholesky jitter retries
    included)."""
    s2, c, rho = theta[0], theta[1], theta[2]
    ls = torch.nn.functional.softplus(rho)
    n = Zn.shape[0]
    eye = torch.eye(n, dtype=torch.float64)
    K = O.kernel_matrix(Zn, Zn, ls) + s2 * eye
    L, info = torch.linalg.cholesky_ex(K)
    jitter, tries = O.CHOLESKY_JITTER, 0
    while int(info) != 0:
        if tries == 3:
            raise RuntimeError("not positive definite after jitter retries")
        L, info = torch.linalg.cholesky_ex(K + jitter * eye)
        jitter, tries = jitter * 10.0, tries + 1
    diff = (ys - c).unsqueeze(-1)
    alpha = torch.cholesky_solve(diff, L)
    log_n = -0.5 * (diff * alpha).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * LOG2PI
    log_prior = torch.distributions.LogNormal(torch.tensor(-4.0, dtype=torch.float64),
                                              torch.tensor(1.0, dtype=torch.float64)).log_prob(s2)
    return -(log_n + log_prior) / n


class RestatedFit:
    """Loss, gradient and scipy fit of one state (Z: n x k reduced points, y: raw objective values)."""

    def __init__(self, Z, y, norm_bounds=None):
        gp = O.ExactGP(Z, y, norm_bounds)
        self.Zn, self.ys, self.n = gp.Zn, gp.y_s, gp.n

    def value_and_grad(self, theta):
        th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
        loss = restated_loss(self.Zn, self.ys, th)
        (g,) = torch.autograd.grad(loss, th)
        return float(loss.detach()), g.numpy().copy()

    def term_scales(self, theta):
        """Per gradient component, the sum of absolute values of the terms it adds up (cancellation near an optimum)."""
        s2, c, rho = (float(v) for v in theta)
        ls = math.log1p(math.exp(rho)) if rho <= 20.0 else rho
        with torch.no_grad():
            K = O.kernel_matrix(self.Zn, self.Zn, ls) + s2 * torch.eye(self.n, dtype=torch.float64)
            Kinv = torch.cholesky_inverse(torch.linalg.cholesky(K))
            alpha = Kinv @ (self.ys - c)
            a = (self.Zn - self.Zn.mean(0)) / ls
            sq = torch.cdist(a, a).pow(2)
            dist = sq.clamp_min(1e-30).sqrt()
            dK = (5.0 / 3.0) * sq * (1.0 + math.sqrt(5.0) * dist) * torch.exp(-math.sqrt(5.0) * dist)
            dK.fill_diagonal_(0.0)
            W = torch.outer(alpha, alpha).abs() + Kinv.abs()
            sig = 1.0 / (1.0 + math.exp(-rho))
            lz = math.log(s2)
            return np.array([
                (0.5 * float((alpha * alpha).sum()) + 0.5 * float(torch.trace(Kinv)) + abs(1.0 + (lz + 4.0)) / s2) / self.n,
                float(alpha.abs().sum()) / self.n,
                0.5 * float((W * dK).sum()) * sig / ls / self.n])

    def fit(self, theta0=THETA0):
        from scipy.optimize import minimize
        return minimize(self.value_and_grad, np.array(theta0, dtype=np.float64), jac=True, method="L-BFGS-B",
                        bounds=[(NOISE_LB, None), (None, None), (None, None)])


def projected_gradient(x, g):
    pg = np.array(g, dtype=np.float64)
    if x[0] <= NOISE_LB and pg[0] > 0.0:                 # at the noise bound a pushing-out gradient is not a descent direction
        pg[0] = 0.0
    return float(np.abs(pg).max())


def seeded_state(seed: int, n: int, k: int):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-2.0, 2.0, size=(n, k))
    y = np.sin(3.0 * Z[:, 0]) + 0.5 * (Z ** 2).sum(1) + 0.1 * rng.standard_normal(n)
    return Z, y


@pytest.mark.parametrize("seed,n,k", [(1, 24, 2), (2, 40, 5), (3, 60, 3)])
def test_restated_gradient_matches_central_differences(seed, n, k):
    torch.set_num_threads(1)
    fit = RestatedFit(*seeded_state(seed, n, k))
    for theta in (THETA0, (1e-4, 0.3, -0.5), (0.05, -0.2, 0.8)):
        _, g = fit.value_and_grad(theta)
        for i in range(3):
            h = 1e-5 * theta[0] if i == 0 else 1e-6      # (the noise: a step relative to its value, inside its domain)
            tp, tm = list(theta), list(theta)
            tp[i] += h
            tm[i] -= h
            fd = (fit.value_and_grad(tp)[0] - fit.value_and_grad(tm)[0]) / (2.0 * h)
            assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])), (seed, theta, i, fd, g[i])


@pytest.mark.parametrize("seed,n,k", [(4, 30, 2), (5, 50, 4)])
def test_restated_scipy_fit_reaches_a_stationary_point(seed, n, k):
    torch.set_num_threads(1)
    fit = RestatedFit(*seeded_state(seed, n, k))
    res = fit.fit()
    assert res.success, res.message
    assert projected_gradient(res.x, res.jac) <= 1e-5, (res.x, res.jac)
    assert res.fun < fit.value_and_grad(THETA0)[0]


def test_fit_gp_with_batched_runs_is_refused(native):
    from Algorithms import ExperimentRunner
    with pytest.raises(ValueError, match="batched"):
        ExperimentRunner(algorithms=["pca"], dimensions=[10], problem_ids=[15], num_runs=30, progress=False,
                         batched=30, fit_gp=True)


def test_main_parses_fit_gp(native):
    spec = importlib.util.spec_from_file_location("pcabo_main_cli", os.path.join(ROOT, "para-ortho-pca-bo_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    saved = os.environ.get("GPU_MAX_HW_QUEUES")          # (main.py sets a default for the processes it drives)
    try:
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            os.environ.pop("GPU_MAX_HW_QUEUES", None)
        else:
            os.environ["GPU_MAX_HW_QUEUES"] = saved
    assert mod.parse_arguments(["--fit_gp"]).fit_gp is True
    assert mod.parse_arguments([]).fit_gp is False


def test_fit_symbols_declared_and_exported(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    for name in ("pcabo_gp_mll", "pcabo_gp_fit"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in native.EXPORTS
        assert hasattr(native.LIB, name)
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2
