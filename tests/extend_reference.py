"""Appending points to a conditioned GP (pcabo_gp_extend / pcabo_gp_truncate): the fantasy model on the oracle, the bordering step
in extended precision, and the error units an fp64 evaluation of that step is judged in.

No tests here: `test_extend_cpu.py` proves the bordering against a refit and the units on a plain numpy restatement,
`test_gpu_extend.py` judges `k_ext_ks`, `k_ext_append` and `k_ext_truncate` (kernels_ext.hip) by them.

The model (include/pcabo.h, `pcabo_gp_extend`): botorch's condition_on_observations.  Transforms and hyperparameters are HELD - the
Normalize bounds (lo, hi), the Standardize statistics (m', s), the lengthscale l, the noise s2, the jitter rung the factorisation
ended on - and only the data grow.  `extended` states it on the oracle's ExactGP: a fresh factorisation of the n + p points with
those held.  The bordering step states the same for one point x with value y on the state {R = L^-1, alpha, y_s}:
  xn = (x - lo) / (hi - lo),  ks_j = k(|xn - zn_j|^2 / l^2) for j < n  (the direct form),
  v = R ks,  w = R^T v,  d2 = (1 + s2 + rung) - |v|^2,  d = sqrt(d2),
  L[n] = [v, d],  R[n] = [-w / d, 1 / d],  ys_n = (y - m') / s   (believer mode: ys_n = alpha . ks),  alpha = R^T (R y_s).
That [v, d] is the next row of the Cholesky factor is the factor's own recurrence (L v = ks, d^2 = K_nn - |v|^2), and
[-w / d, 1 / d] is the next row of its inverse because L[n] R = e_n reads v^T R + d r = 0 with R = L^-1 of the leading block.

Error units: first-order bounds of what ANY fp64 evaluation of the step commits, eps = 2^-52 (twice the unit roundoff: every count
below is generous by that factor), computed from the reference's own quantities, never from a run of the code under test.  |.| is
elementwise, n the number of points before the step.

Kernel vector (`ks_units`, the direct form, as acq_reference's dks).  xn_c and zn_jc are each a subtraction, the rounded range and
a division: 2 eps relative.  d_c = xn_c - zn_jc:  dd_c = 2 eps (|xn_c| + |zn_jc|) + eps |d_c|.  The k-term sum of squares, 1 / l, its
square and the product:  dsq = (2 sum_c |d_c| dd_c + (k + 2) eps sum_c d_c^2) / l^2 + 3 eps sq.  The map:
  u_ks = |dk/dsq|(max(sq - dsq, 0)) dsq + eps ks (4 + arg),   |dk/dsq| = 5/6 (1 + sqrt5 r) exp(-sqrt5 r), arg = sqrt5 r   (Matern)
                                                              or ks / 2, sq / 2   (RBF).
Rows on a GIVEN R (`step(...).units`; the device test applies the reference to the device's own R, so the inverse's residual is not in
play there).  Row p of v is a sum of p + 1 products in some order, (p + 1) eps / 2 <= n eps of its absolute terms, plus the kernel
vector's own error carried through:
  u_v  = n eps |R||ks| + |R| u_ks
  u_w  = n eps |R^T||v| + |R^T| u_v                       (w = R^T v, column sums of at most n terms)
  u_d2 = (n + 2) eps (1 + s2 + rung) + 2 |v| . u_v       (the two additions of the diagonal, n squares and their sum - bounded by the
                                                          diagonal because |v|^2 < 1 + s2 + rung - and the subtraction)
  u_d  = u_d2 / (2 d) + eps d                             (the square root)
  new row of L: [u_v, u_d];   new row of R: u_w / d + |w| u_d / d^2 + eps |w| / d,  and  u_d / d^2 + eps / d  on the diagonal.
Rows against the EXACT factor (`row_units_refit`).  The stored R~ is a computed inverse, L R~ = I + F with |F| <= u_R =
n eps |L||R| + the block term of gp_reference (multiplying by an explicit inverse is only as good as that inverse's residual, which
is why this is not Higham's (n + 1) eps of a substitution), and L~ = L + dL with |dL| <= |L| tril(|R| u_C |R^T|), the factor's own
first-order forward error.  Then R~ = L~^-1 (I + F) = R - R dL R + R F to first order, |R~ - R| <= |R| (u_R + |dL||R|), and
  u_v' = u_v + |R| (u_R + |dL||R|) |ks|,
the rest of the chain as above with u_v' for u_v; all from gp_reference's units of the n points.
alpha on a given R (`alpha_units`): t = R y_s and alpha = R^T t, n-term sums each, and the new entry of y_s (2 eps |ys_n|; believer
mode: n eps sum |alpha_j ks_j| + |alpha| . u_ks):
  u_alpha = n eps (|R^T||R||y_s| + |R^T||t|) + |R^T||R| u_ys.
The limit is 16 units, as in the other edge tests.
"""
import math
from types import SimpleNamespace

import numpy as np

import gp_reference as G
from wpca_reference import EPS, f64, hp, hp_sqrt

LIMIT = 16.0
_S5 = math.sqrt(5.0)


# ---- the fantasy model on the oracle ---------------------------------------------------------------------------------------------
def extended(gp, Z, Xp, yp=None):
    """The oracle's ExactGP on the n + p points (Z, Xp) with gp's Normalize bounds, hyperparameters and Standardize statistics held
    (posterior_reference.conditioned_on_one_more for p points and with targets).  y_s = (y - m') / s for the new points, or with
    yp = None (believer mode) the posterior mean of the model before each point, one after the other."""
    import torch
    import pcabo_oracle as O
    Z = np.asarray(Z, dtype=np.float64)
    Xp = np.asarray(Xp, dtype=np.float64).reshape(-1, Z.shape[1])

    def held(points, ys):
        g = O.ExactGP(points, np.zeros(points.shape[0]), gp.norm_bounds, lengthscale=gp.lengthscale, noise=gp.noise, kernel=gp.kernel)
        g.y_mean, g.y_std, g.y_s = gp.y_mean, gp.y_std, ys
        return g

    ys = gp.y_s.clone()
    if yp is not None:
        new = (torch.from_numpy(np.asarray(yp, dtype=np.float64).reshape(-1)) - gp.y_mean.view(())) / gp.y_std.view(())
        return held(np.vstack([Z, Xp]), torch.cat([ys, new]))
    for i in range(Xp.shape[0]):
        g = held(np.vstack([Z, Xp[:i]]), ys)
        g.condition()
        xn = g._normalize(torch.from_numpy(Xp[i:i + 1].copy()))
        ks = O.kernel_matrix(xn, g.Zn, g.lengthscale, g.kernel)
        ys = torch.cat([ys, (ks @ g.alpha).reshape(1)])
    return held(np.vstack([Z, Xp]), ys)


# ---- the bordering step in extended precision --------------------------------------------------------------------------------------
def _cov(sq, kernel):
    """k, |dk/dsq| and the exponential's argument of a scaled squared distance (any float type)."""
    if kernel == "rbf":
        ks = G.hp_exp(-sq / 2)
        return ks, ks / 2, sq / 2
    r, s5 = hp_sqrt(sq), hp_sqrt(hp(5.0))
    e = G.hp_exp(-s5 * r)
    return (1 + s5 * r + hp(5.0) / hp(3.0) * sq) * e, hp(5.0) / hp(6.0) * (1 + s5 * r) * e, s5 * r


def kernel_vector(x, Z, bounds, lengthscale, kernel):
    """ks (n, extended precision) of the point x against the points Z with the held bounds (2 x k), and its unit u_ks (fp64)."""
    lo, hi = hp(bounds[0]), hp(bounds[1])
    span = hi - lo
    xn, zn = (hp(x) - lo) / span, (hp(Z) - lo) / span
    d = xn[None, :] - zn
    ssq = (d * d).sum(axis=1)
    ls = float(lengthscale)
    sq = ssq / (hp(ls) * hp(ls))
    ks, dks_dsq, arg = _cov(sq, kernel)
    D, k = np.abs(f64(d)), Z.shape[1]
    dd = 2.0 * EPS * (np.abs(f64(xn))[None, :] + np.abs(f64(zn))) + EPS * D
    dsq = (2.0 * (D * dd).sum(axis=1) + (k + 2) * EPS * f64(ssq)) / (ls * ls) + 3.0 * EPS * f64(sq)
    sq_lo = hp(np.maximum(f64(sq) - dsq, 0.0))
    slope = np.maximum(f64(_cov(sq_lo, kernel)[1]), f64(dks_dsq))
    return ks, slope * dsq + EPS * np.abs(f64(ks)) * (4.0 + f64(arg)), xn


def kernel_vector_f64(x, Z, bounds, lengthscale, kernel):
    """The kernel vector in plain fp64 numpy, written as the kernels are (direct form, 1 / l squared, the 1e-30 guard)."""
    lo, hi = np.asarray(bounds[0], dtype=np.float64), np.asarray(bounds[1], dtype=np.float64)
    xn, zn = (np.asarray(x, dtype=np.float64) - lo) / (hi - lo), (np.asarray(Z, dtype=np.float64) - lo) / (hi - lo)
    d = xn[None, :] - zn
    il = 1.0 / float(lengthscale)
    sq = (d * d).sum(axis=1) * (il * il)
    if kernel == "rbf":
        return np.exp(-0.5 * sq)
    r = np.sqrt(np.maximum(sq, 1e-30))
    return ((_S5 * r + 1.0) + (5.0 / 3.0) * (r * r)) * np.exp(-_S5 * r)


# ---- the inputs of the tests: shapes and new points ----------------------------------------------------------------------------------
KINDS = ("uniform", "outside", "copy0", "near1")
# (n, p): the smallest shapes at which the kernels can go wrong - a partial block, the last row of a block (NP stays), the first row
# of a new block (NP grows: the padding is written), the row behind it, a call that crosses a block in its middle, two blocks
SHAPES = ((2, 1), (63, 1), (64, 1), (65, 1), (127, 3), (129, 1))
GPU_K = (1, 5, 33, 65)


def gpu_cases():
    """[(n, p, k, hyper, kinds)] of the device test: SHAPES x GPU_K with the default hyperparameters (Matern), RBF at two of them;
    the kinds of new points rotate so that every kind meets every shape."""
    out, i = [], 0
    for n, p in SHAPES:
        for k in GPU_K:
            out.append((n, p, k, "default", tuple(KINDS[(i + j) % 4] for j in range(p))))
            i += 1
    out.append((64, 1, 5, "rbf", ("copy0",)))
    out.append((127, 3, 5, "rbf", ("near1", "uniform", "outside")))
    return out


def held_of(case):
    """(bounds, m', s) of the n points in plain fp64, as pcabo_gp_condition states them: what a CPU test holds fixed (the device
    test holds the device's own)."""
    Z, y = case.Z, case.y
    if case.norm_bounds is None:
        zmin, zmax = Z.min(axis=0), Z.max(axis=0)
        bounds = np.vstack([zmin - 0.1 * (zmax - zmin), zmax + 0.1 * (zmax - zmin)])
    else:
        bounds = np.asarray(case.norm_bounds, dtype=np.float64)
    m = y.sum() / len(y)
    s = math.sqrt(((y - m) ** 2).sum() / (len(y) - 1))
    return bounds, m, s if s >= 1e-8 else 1.0


def new_points(case, bounds, kinds):
    """p new points (p x k) and their values: a uniform draw from the data's range, a point outside the Normalize box by 0.3 of its
    range in every coordinate, an exact copy of training point 0, training point 1 moved by 1e-9."""
    rng = np.random.default_rng([case.n, case.k, len(kinds), KINDS.index(kinds[0]), 911])
    lo, hi = np.asarray(bounds[0]), np.asarray(bounds[1])
    rows = []
    for kind in kinds:
        if kind == "uniform":
            rows.append(rng.uniform(case.Z.min(axis=0), case.Z.max(axis=0)))
        elif kind == "outside":
            rows.append(hi + 0.3 * (hi - lo))
        elif kind == "copy0":
            rows.append(case.Z[0].copy())
        else:
            rows.append(case.Z[1] + 1e-9)
    return np.ascontiguousarray(np.vstack(rows)), rng.normal(size=len(kinds)) * 200.0 + 900.0


def border(R, ks, diag):
    """One bordering step on R (n x n lower, taken as exact) with the kernel vector ks and the diagonal 1 + s2 + rung, in extended
    precision: v, w, d2, d and the new rows of L and R (n + 1 entries each)."""
    Rh, kh = np.tril(hp(R)), hp(ks)
    v = Rh @ kh
    w = Rh.T @ v
    d2 = hp(diag) - (v * v).sum()
    if not d2 > 0:
        raise G.NotPositiveDefinite("d2 = %r" % float(d2))
    d = hp_sqrt(d2)
    one = hp(np.ones(1))
    return SimpleNamespace(v=v, w=w, d2=d2, d=d, L_row=np.concatenate([v, d * one]), R_row=np.concatenate([-w / d, one / d]))


def border_f64(R, ks, diag):
    """The same step in plain fp64 numpy: what the units must hold for.  d2 <= 0 or not finite: None."""
    R, ks = np.tril(np.asarray(R, dtype=np.float64)), np.asarray(ks, dtype=np.float64)
    v = R @ ks
    w = R.T @ v
    d2 = float(diag) - float((v * v).sum())
    if not (d2 > 0.0 and math.isfinite(d2)):
        return None
    d = math.sqrt(d2)
    return SimpleNamespace(v=v, w=w, d2=d2, d=d, L_row=np.append(v, d), R_row=np.append(-w / d, 1.0 / d))


def _row_units(aR, n, b, u_ks, diag, extra_v):
    """Units of the new rows of L and R (n + 1 entries each), of d2 and of v from a `border` result b (with b.ks_abs = |ks|) on a
    matrix with absolute values aR; extra_v: what the matrix's own error adds to u_v (row_units_refit)."""
    v, w, d = np.abs(f64(b.v)), np.abs(f64(b.w)), float(b.d)
    u_v = n * EPS * (aR @ b.ks_abs) + aR @ u_ks
    if extra_v is not None:
        u_v = u_v + extra_v
    u_w = n * EPS * (aR.T @ v) + aR.T @ u_v
    u_d2 = (n + 2) * EPS * float(diag) + 2.0 * float(v @ u_v)
    u_d = u_d2 / (2.0 * d) + EPS * d
    u_L = np.append(u_v, u_d)
    u_R = np.append(u_w / d + w * u_d / (d * d) + EPS * w / d, u_d / (d * d) + EPS / d)
    return SimpleNamespace(L_row=u_L, R_row=u_R, d2=u_d2, v=u_v)


def step(R, x, Z, bounds, lengthscale, noise, kernel, rung=0.0):
    """kernel_vector + border + row_units of one point on a given R: the reference of one appended row."""
    ks, u_ks, xn = kernel_vector(x, Z, bounds, lengthscale, kernel)
    diag = hp(1.0) + hp(noise) + hp(rung)
    b = border(R, ks, diag)
    b.ks, b.ks_abs, b.u_ks, b.xn, b.diag = ks, np.abs(f64(ks)), u_ks, xn, diag
    b.units = _row_units(np.abs(np.tril(f64(R))), np.asarray(R).shape[0], b, u_ks, float(diag), None)
    return b


def row_units_refit(ref, b):
    """Units of the new row of L against the EXACT factor's row, where the R the step ran on is a computed inverse of a computed
    factor: ref = gp_reference.reference of the n points (its u_R, u_C, L, R), b = a `step` result on that R."""
    aL, aR = np.abs(f64(ref.L)), np.abs(f64(ref.R))
    n = aR.shape[0]
    dL = aL @ np.tril(aR @ ref.u_C @ aR.T)                       # first-order forward error of the factor
    extra = aR @ ((ref.u_R + dL @ aR) @ b.ks_abs)
    return _row_units(aR, n, b, b.u_ks, float(b.diag), extra)


def alpha_units(R, ys, u_ys_new):
    """Units of alpha = R^T (R y_s) on a given R and y_s (n + p entries), u_ys_new (p) the units of the appended entries of y_s."""
    aR = np.abs(np.tril(f64(R)))
    n = aR.shape[0]
    Rh, yh = np.tril(hp(R)), hp(ys)
    t = Rh @ yh
    alpha = Rh.T @ t
    u_ys = np.zeros(n)
    u_ys[n - len(u_ys_new):] = u_ys_new
    unit = n * EPS * (aR.T @ (aR @ np.abs(f64(yh))) + aR.T @ np.abs(f64(t))) + aR.T @ (aR @ u_ys)
    return alpha, unit


def ratio(err, unit):
    return G._ratio(err, unit)


# ---- the whole extended model in extended precision and in plain fp64 -------------------------------------------------------------
def extended_case(case, Xp, yp, bounds):
    """gp_reference's case of the n + p points with the held bounds as user bounds (yp = None: the new targets are placeholders)."""
    Xp = np.asarray(Xp, dtype=np.float64).reshape(-1, case.k)
    y_new = np.zeros(Xp.shape[0]) if yp is None else np.asarray(yp, dtype=np.float64).reshape(-1)
    return SimpleNamespace(Z=np.ascontiguousarray(np.vstack([case.Z, Xp])), y=np.concatenate([case.y, y_new]), n=case.n + Xp.shape[0],
                           k=case.k, lengthscale=case.lengthscale, noise=case.noise, kernel=case.kernel,
                           norm_bounds=np.asarray(bounds, dtype=np.float64), gen=case.gen, hyper=case.hyper, id=case.id + "+%d" % Xp.shape[0])


def _believer_targets(K, ys_n, n, p, solve):
    ys = ys_n
    for i in range(p):
        m = n + i
        ys = np.concatenate([ys, (K[m, :m] @ solve(K[:m, :m], ys)).reshape(1)])
    return ys


def reference_state(case, Xp, yp, held):
    """The extended model by a fresh factorisation of the n + p points in extended precision, the held transforms fixed:
    held = (bounds 2 x k, m', s) as fp64 numbers.  yp = None: believer mode.  K, L, R, alpha, ys and the state dict acq_reference's
    `linear` takes."""
    bounds, m, s = held
    ec = extended_case(case, Xp, yp, bounds)
    g = G.gram_reference(ec)
    assert g.skip is None, g.skip
    n, p = case.n, ec.n - case.n
    ys = (hp(ec.y) - hp(m)) / hp(s)
    if yp is None:
        def solve(Kb, yb):
            f = G.factor_reference(Kb, yb)
            return f.alpha
        ys = _believer_targets(g.K, ys[:n], n, p, solve)
    fr = G.factor_reference(g.K, ys)
    gs = {"R": fr.R, "alpha": fr.alpha, "y_mean": float(m), "y_std": float(s), "norm_bounds": np.asarray(bounds, dtype=np.float64)}
    return SimpleNamespace(case=ec, K=g.K, L=fr.L, R=fr.R, alpha=fr.alpha, ys=ys, gs=gs, m=float(m), s=float(s))


def restated_state(case, Xp, yp, held):
    """The same in plain fp64 numpy / LAPACK (gp_reference.restate: norms + GEMM distance, numpy's Cholesky, a triangular solve for
    R, two mat-vecs for alpha) with the held statistics: the yardstick of the end-to-end comparison."""
    bounds, m, s = held
    ec = extended_case(case, Xp, yp, bounds)
    r = G.restate(ec)
    n, p = case.n, ec.n - case.n
    ys = (ec.y - m) / s
    if yp is None:
        ys = _believer_targets(r.K, ys[:n], n, p, lambda Kb, yb: np.linalg.solve(Kb, yb))
    alpha = r.R.T @ (r.R @ ys)
    gs = {"R": r.R, "alpha": alpha, "y_mean": float(m), "y_std": float(s), "norm_bounds": np.asarray(bounds, dtype=np.float64)}
    return SimpleNamespace(case=ec, K=r.K, L=r.L, R=r.R, alpha=alpha, ys=ys, gs=gs, m=float(m), s=float(s))


def acq_state(ec):
    """The inputs of acq_reference.linear / restate for an extended case."""
    return SimpleNamespace(Z=ec.Z, k=ec.k, n=ec.n, lengthscale=ec.lengthscale, kernel="rbf" if ec.kernel == "rbf" else "matern52")


def posterior(state, X):
    """mean, variance (not floored) and covariance at X of a reference_state (extended precision) or a restated_state (fp64): the
    statement of posterior_reference on the state's own R and alpha."""
    ec, gs = state.case, state.gs
    ext = np.asarray(gs["R"]).dtype == np.longdouble
    cast = hp if ext else (lambda a: np.asarray(a, dtype=np.float64))
    lo, hi = cast(gs["norm_bounds"][0]), cast(gs["norm_bounds"][1])
    xn, zn = (cast(X) - lo) / (hi - lo), (cast(ec.Z) - lo) / (hi - lo)
    ls2 = cast(ec.lengthscale) * cast(ec.lengthscale)

    def cov_of(a, b):
        d = a[:, None, :] - b[None, :, :]
        sq = (d * d).sum(axis=2) / ls2
        if ext:
            return _cov(sq, ec.kernel)[0]
        if ec.kernel == "rbf":
            return np.exp(-0.5 * sq)
        r = np.sqrt(np.maximum(sq, 1e-30))
        return ((_S5 * r + 1.0) + (5.0 / 3.0) * (r * r)) * np.exp(-_S5 * r)

    ks = cov_of(xn, zn)
    R, alpha = np.tril(cast(gs["R"])), cast(gs["alpha"])
    V = ks @ R.T
    prior = cov_of(xn, xn)
    s = cast(state.s)
    cov = (prior - V @ V.T) * (s * s)
    return {"mean": cast(state.m) + s * (ks @ alpha), "variance": np.diagonal(cov).copy(), "covariance": cov}
