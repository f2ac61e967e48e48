"""The restated GP fit with one lengthscale per input (ARD), host side: what pcabo_gp_mll_ard / pcabo_gp_fit_ard are checked against.

The model of tests/test_gp_fit_cpu.py with MaternKernel(nu=2.5, ard_num_dims=k):

    loss(theta) = -[log N(y_s; c 1, K_l + s2 I) + log LogNormal(s2; -4, 1)] / n,   theta = (s2, c, rho_1 .. rho_k), l_c = softplus(rho_c)

through torch float64 autograd (the oracle's kernel_matrix broadcasts a vector lengthscale over the last axis) and scipy's L-BFGS-B
with its defaults (ArdFit.fit; with rho_min=RHO_MIN it has the one bound the device fit adds).  Equal rho is exactly the scalar
restatement.  As for the scalar fit, BoTorch / GPyTorch are not installed here,
so parity with them is not pinned (DESIGN.md "ARD lengthscales").
"""
import math

import numpy as np
import torch

import pcabo_oracle as O
from test_gp_fit_cpu import LOG2PI, NOISE_LB, THETA0

FIT_STATES = [(1, 40, 3), (2, 65, 5), (4, 70, 33)]       # (seed, n, k) of the states whose fits the tests compare
EVAL_ONLY_STATE = (3, 130, 9)                            # its reference fit leaves the domain: evaluations only
RHO_MIN = -40.0 * math.log(2.0)                          # the device fit's lower bound on every rho_c (FIT_ARD_RHO_MIN, host_side.h)


def ard_state(seed: int, n: int, k: int):
    """Z ~ U(-2, 2)^k, y = sin(3 z0) + 0.5 (z0^2 + z1^2) + 0.1 eps: only the first two inputs matter (the first alone at k = 1)."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-2.0, 2.0, size=(n, k))
    y = np.sin(3.0 * Z[:, 0]) + 0.5 * (Z[:, :2] ** 2).sum(1) + 0.1 * rng.standard_normal(n)
    return Z, y


def theta0(k: int) -> np.ndarray:
    return np.array([THETA0[0], THETA0[1]] + [0.0] * k, dtype=np.float64)


def softplus(rho) -> np.ndarray:
    """torch.nn.functional.softplus in float64 (threshold 20)."""
    return torch.nn.functional.softplus(torch.as_tensor(np.asarray(rho, dtype=np.float64))).numpy()


def ard_loss(Zn: torch.Tensor, ys: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """restated_loss of tests/test_gp_fit_cpu.py with a vector lengthscale (jitter retries included)."""
    s2, c, rho = theta[0], theta[1], theta[2:]
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


class ArdFit:
    """Loss, gradient, term scales and scipy fit of one state (Z: n x k points, y: raw objective values)."""

    def __init__(self, Z, y, norm_bounds=None):
        gp = O.ExactGP(Z, y, norm_bounds)
        self.Zn, self.ys, self.n, self.k = gp.Zn, gp.y_s, gp.n, gp.k

    def value_and_grad(self, theta):
        th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
        loss = ard_loss(self.Zn, self.ys, th)
        (g,) = torch.autograd.grad(loss, th)
        return float(loss.detach()), g.numpy().copy()

    def term_scales(self, theta):
        """Per gradient component, the sum of absolute values of the terms it adds up (RestatedFit.term_scales, with |dK_c| per
        input: dK/dlog l_c = (5/3) (1 + sqrt5 r) exp(-sqrt5 r) (a_ci - a_cj)^2)."""
        theta = np.asarray(theta, dtype=np.float64)
        s2, c, rho = float(theta[0]), float(theta[1]), theta[2:]
        ls = torch.from_numpy(softplus(rho))
        with torch.no_grad():
            K = O.kernel_matrix(self.Zn, self.Zn, ls) + s2 * torch.eye(self.n, dtype=torch.float64)
            Kinv = torch.cholesky_inverse(torch.linalg.cholesky(K))
            alpha = Kinv @ (self.ys - c)
            a = (self.Zn - self.Zn.mean(0)) / ls
            dist = torch.cdist(a, a).pow(2).clamp_min(1e-30).sqrt()
            G = (5.0 / 3.0) * (1.0 + math.sqrt(5.0) * dist) * torch.exp(-math.sqrt(5.0) * dist)
            G.fill_diagonal_(0.0)
            W = (torch.outer(alpha, alpha).abs() + Kinv.abs()) * G
            sig = 1.0 / (1.0 + np.exp(-rho))
            lz = math.log(s2)
            out = np.empty(2 + self.k)
            out[0] = (0.5 * float((alpha * alpha).sum()) + 0.5 * float(torch.trace(Kinv)) + abs(1.0 + (lz + 4.0)) / s2) / self.n
            out[1] = float(alpha.abs().sum()) / self.n
            for j in range(self.k):
                d2 = (a[:, j, None] - a[None, :, j]).pow(2)
                out[2 + j] = 0.5 * float((W * d2).sum()) * sig[j] / float(ls[j]) / self.n
            return out

    def fit(self, start=None, rho_min=None):
        """scipy's fit of the model as stated (rho unbounded); rho_min=RHO_MIN restates the device fit's lower bound on every rho_c."""
        from scipy.optimize import minimize
        start = theta0(self.k) if start is None else np.array(start, dtype=np.float64)
        return minimize(self.value_and_grad, start, jac=True, method="L-BFGS-B",
                        bounds=[(NOISE_LB, None), (None, None)] + [(rho_min, None)] * self.k)


def fitted_gp(Z, y, hp, norm_bounds=None) -> "O.ExactGP":
    """The oracle's exact GP at a fit's result (its dict): a vector lengthscale and the mean constant as m' = m + s c."""
    gp = O.ExactGP(Z, y, norm_bounds, lengthscale=torch.tensor(np.asarray(hp["lengthscales"], dtype=np.float64)), noise=hp["noise"])
    gp.y_mean = gp.y_mean + gp.y_std * hp["mean_constant"]
    gp.y_s = gp.y_s - hp["mean_constant"]
    return gp
