"""Leave-one-out (LOO) predictions of the conditioned GP: the closed form in extended precision, a brute-force refit to prove it,
and the error units an fp64 evaluation of the closed form is judged in.

No tests here: `test_loo_cpu.py` proves the closed form against the brute force and the units on a plain numpy restatement,
`test_gpu_loo.py` judges `k_loo` (pcabo_gp_loo / pcabo_batch_gp_loo) by them.

The closed form (include/pcabo.h, `pcabo_gp_loo`; Rasmussen & Williams 5.4.2).  With R = L^-1 the root inverse of the factored K,
alpha = K^-1 y_s, y_s = (y - m') / s the standardised targets and (m', s) the Standardize statistics (after a fit m' = m + s c
carries the constant mean c):
  d_i    = sum_{p >= i} R[p][i]^2       = (K^-1)_ii
  r_i    = alpha_i / d_i
  mean_i = m' + s (ys_i - r_i)
  var_i  = s^2 / d_i
  z_i    = r_i sqrt(d_i)
  lpd_i  = -1/2 (log(2 pi) + log(var_i) + z_i^2)
The hyperparameters and the Standardize / Normalize statistics are those of the FULL data: the LOO identity, not a refit of the
transforms.  `brute_force` is that statement without the identity: K, y_s, m' and s of the full data in extended precision
(`gp_reference.gram_reference`), then for every i the other n - 1 points factored and solved on their own,
  mean_i = m' + s k_i^T K_-i^-1 ys_-i,   var_i = s^2 (K_ii - k_i^T K_-i^-1 k_i),   z_i = (y_i - mean_i) / sqrt(var_i).

Error units (`units`): first-order bounds of what ANY fp64 evaluation of the closed form commits on GIVEN R, alpha, y and (m', s),
u = 2^-53 the unit roundoff.  All come from the reference's own values (closed_form in extended precision); nothing comes from a
run of the code under test.  n is the number of points.
  d     a sum of at most n non-negative rounded squares, in any order (with or without fused multiply-add): the squares 1 u
        each, the additions at most n - 1 u on a sum of non-negative terms - relative (n + 1) u.
  r     d and one division: relative (n + 2) u.
  var   s^2 (1 u), d and one division: relative (n + 3) u.
  z     r, the square root of d ((n + 1) / 2 + 1 u) and one product: relative (1.5 n + 5) u, absolute at |z_i|.
  mean  ys_i = (y_i - m') / s is formed in fp64 (2 u, a multiplication by the reciprocal would be 3 u), the subtraction of r_i
        (1 u at |ys_i| + |r_i|), the product with s and the addition of m' (1 u each at the size of their results), r's own error
        s (n + 2) u |r_i|:  u ((n + 5) s |r_i| + 6 (|m'| + s |ys_i|)) - a small number of roundings at the size of
        |m'| + s |ys_i|, and r_i's inherited error at its own size.
  lpd   absolute: the logarithm's argument ((n + 3) u relative in var is (n + 3) u absolute in the logarithm), the logarithm
        itself (4 ulp = 8 u at |log var_i|), the square of z (2 (1.5 n + 5) + 1 u at z_i^2), the two additions (2 u at the size of
        the terms); the halving is exact:
        u / 2 ((n + 3) + 8 |log var_i| + (3 n + 11) z_i^2 + 2 (log(2 pi) + |log var_i| + z_i^2)).
The limit is 16 units, as in the other edge tests.
"""
import math
from types import SimpleNamespace

import numpy as np

from gp_reference import factor_reference, gram_reference, hp_cholesky, restate
from wpca_reference import f64, hp, hp_log, hp_sqrt

U = 2.0 ** -53                   # unit roundoff of fp64
LIMIT = 16.0
LOG2PI = math.log(2.0 * math.pi)
KEYS = ("mean", "variance", "z", "lpd")


def closed_form(R, alpha, y, ystats):
    """mean, variance, z, lpd (and d, r, ys) of the definition in np.longdouble from R (n x n, lower), alpha (n), the raw targets
    y (n) and ystats = (m', s)."""
    Rh, ah, yh = np.tril(hp(R)), hp(alpha), hp(y)
    m, s = hp(ystats[0]), hp(ystats[1])
    ys = (yh - m) / s
    d = (Rh * Rh).sum(axis=0)
    r = ah / d
    var = s * s / d
    z = r * hp_sqrt(d)
    lpd = -(hp(LOG2PI) + hp_log(var) + z * z) / 2
    return SimpleNamespace(mean=m + s * (ys - r), variance=var, z=z, lpd=lpd, d=d, r=r, ys=ys, m=m, s=s, n=len(yh))


def closed_form_f64(R, alpha, y, ystats):
    """The closed form in plain fp64 numpy: what the units must hold for."""
    R, alpha, y = np.tril(np.asarray(R, dtype=np.float64)), np.asarray(alpha, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m, s = float(ystats[0]), float(ystats[1])
    ys = (y - m) / s
    d = (R * R).sum(axis=0)
    r = alpha / d
    z = r * np.sqrt(d)
    var = s * s / d
    return {"mean": m + s * (ys - r), "variance": var, "z": z, "lpd": -0.5 * (LOG2PI + np.log(var) + z * z)}


def units(cf):
    """The error units of the four vectors from a closed_form result (see the module docstring)."""
    n = cf.n
    r, ys, var, z = np.abs(f64(cf.r)), np.abs(f64(cf.ys)), f64(cf.variance), f64(cf.z)
    m, s = abs(float(cf.m)), float(cf.s)
    lv = np.abs(np.log(var))
    return {"mean": U * ((n + 5) * s * r + 6.0 * (m + s * ys)),
            "variance": (n + 3) * U * var,
            "z": (1.5 * n + 5) * U * np.abs(z),
            "lpd": 0.5 * U * ((n + 3) + 8.0 * lv + (3 * n + 11) * z * z + 2.0 * (LOG2PI + lv + z * z))}


def unit_ratios(got, cf):
    """max |got - closed form| / unit per vector (got: a dict with KEYS); NaN or an error at a zero unit counts as infinite."""
    un = units(cf)
    out = {}
    for key in KEYS:
        err = np.abs(f64(hp(got[key]) - getattr(cf, key)))
        if not np.all(np.isfinite(err)) or np.any(err[un[key] == 0.0] != 0.0):
            out[key] = float("inf")
            continue
        pos = un[key] > 0.0
        out[key] = float((err[pos] / un[key][pos]).max()) if pos.any() else 0.0
    return out


# ---- the full chain ----------------------------------------------------------------------------------------------------------
def _mean_c(case):
    return float(getattr(case, "mean_c", 0.0))


def full_reference(case):
    """K, y_s (the mean constant taken off), m' and s of the full data in extended precision, with R and alpha of K."""
    g = gram_reference(case)
    assert g.skip is None, g.skip
    c = hp(_mean_c(case))
    ys = g.ys - c
    fr = factor_reference(g.K, ys)
    return SimpleNamespace(n=g.n, K=g.K, ys=ys, m=g.ym + g.sd * c, s=g.sd, R=fr.R, alpha=fr.alpha)


def _forward(L, B):
    """L^-1 B for a lower-triangular L, extended precision."""
    T = hp(np.zeros(B.shape))
    for j in range(L.shape[0]):
        T[j] = (B[j] - L[j, :j] @ T[:j]) / L[j, j] if j else B[j] / L[j, j]
    return T


def brute_force(case, full=None):
    """mean, variance, z, lpd by a refit without point i for every i, in extended precision, the statistics of the full data
    held fixed (case: gp_reference.make_case's namespace, optionally with mean_c, the constant mean of a fitted model)."""
    full = full_reference(case) if full is None else full
    n, K, ys = full.n, full.K, full.ys
    pm, pv = hp(np.zeros(n)), hp(np.zeros(n))
    for i in range(n):
        keep = np.arange(n) != i
        L = hp_cholesky(K[np.ix_(keep, keep)])
        T = _forward(L, np.stack([ys[keep], K[keep, i]], axis=1))
        pm[i] = T[:, 1] @ T[:, 0]
        pv[i] = K[i, i] - T[:, 1] @ T[:, 1]
    mean = full.m + full.s * pm
    var = full.s * full.s * pv
    z = (hp(case.y) - mean) / hp_sqrt(var)
    return SimpleNamespace(mean=mean, variance=var, z=z, lpd=-(hp(LOG2PI) + hp_log(var) + z * z) / 2, n=n)


def restate_chain(case):
    """The whole chain in plain fp64 numpy (gp_reference.restate: norms + GEMM distance, LAPACK's Cholesky, a triangular solve for
    R, two mat-vecs for alpha), then closed_form_f64: the yardstick of the end-to-end comparison."""
    r = restate(case)
    y = np.asarray(case.y, dtype=np.float64)
    m = r.y_mean + r.y_std * _mean_c(case) if _mean_c(case) != 0.0 else r.y_mean
    ys = (y - m) / r.y_std
    alpha = r.R.T @ (r.R @ ys)
    return closed_form_f64(r.R, alpha, y, (m, r.y_std))


def distances(got, bf):
    """How far a result (dict with KEYS) lies from the brute force, largest over the points: the mean in LOO standard
    deviations, the variance relative, z and lpd absolute."""
    sd = hp_sqrt(bf.variance)
    out = {"mean": np.abs((hp(got["mean"]) - bf.mean) / sd), "variance": np.abs(hp(got["variance"]) / bf.variance - 1),
           "z": np.abs(hp(got["z"]) - bf.z), "lpd": np.abs(hp(got["lpd"]) - bf.lpd)}
    return {key: (float(f64(v).max()) if np.all(np.isfinite(f64(v))) else float("inf")) for key, v in out.items()}
