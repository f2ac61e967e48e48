"""Extended-precision reference of the GP conditioning chain and the error units its results are judged in.

No tests here: `test_gp_reference_cpu.py` proves the reference and its units on a plain numpy restatement,
`test_gpu_gp_edges.py` judges the HIP kernels (`k_zstats`, `k_znorm`, `k_gram`, the Cholesky kernels,
`k_trinv_diag_w`, `k_trinv_cols`, `k_rmatvec`, `k_rtmatvec`) by them.

The chain (include/pcabo.h, `pcabo_gp_condition`), for points Z (n x k), targets y, lengthscale l, noise s2:
  lo, hi = min_i Z -+ 0.1 (max_i Z - min_i Z) per column, or the user's bounds       Normalize
  zn = (Z - lo) / (hi - lo),  a_i = (zn_i - mean_i zn) / l
  sq_ij = sum_c (a_ic - a_jc)^2   - taken DIRECTLY here, never as |a_i|^2 + |a_j|^2 - 2 a_i.a_j
  v = (1 + sqrt5 d + 5/3 d^2) exp(-sqrt5 d), d = sqrt(sq)  (Matern-5/2)   or   exp(-sq / 2)  (RBF);  K = v + s2 I
  y_s = (y - mean y) / sd,  sd = unbiased standard deviation, 1 where it is below 1e-8
  L = chol(K),  R = L^-1,  t = R y_s,  alpha = R^T t
in `np.longdouble` (64-bit mantissa on x86; where it is a plain double the formulas run on `mpmath` objects and
`reference()` refuses n > MP_MAX_N).  A column in which all points agree makes 0 / 0 in zn; the NaN reaches the
Cholesky, which raises `NotPositiveDefinite`.

Error units: first-order bounds of what ANY fp64 implementation of this chain commits (eps = 2^-52).  All are
computed from reference quantities; nothing comes from a run of the code under test.  |.| is elementwise.

K (`u_K`).  Rounding lo and hi moves every point of a column alike (cancels in a_i - a_j) and scales the column
by 1 + delta_c, delta_c = eps ((|lo_c| + |hi_c|) / (2 (hi_c - lo_c)) + 3) (user bounds are exact: 3 eps - the
division, 1 / l and the product).  Each a_ic carries its own e_ic = eps (|zn_ic| / l + |a_ic|) (the subtraction
and the division of zn; the centring and the scaling).  The norm + GEMM form of the distance adds the rounding of
two k-term sums of squares and one k-term dot product, at the size of the terms and not of their difference:
  dsq_ij = 2 sum_c |a_ic - a_jc| (e_ic + e_jc) + 2 sum_c delta_c (a_ic - a_jc)^2
           + (k + 2) eps (nrm_i + nrm_j + 2 sum_c |a_ic a_jc|),                        nrm_i = sum_c a_ic^2
  u_K_ij = |dv/dsq|(max(sq_ij - dsq_ij, 0)) dsq_ij + eps |v_ij| (4 + arg),   u_K_ii = 2 eps (1 + s2)
with |dv/dsq| = 5/6 (1 + sqrt5 d) exp(-sqrt5 d), arg = sqrt5 d (Matern) and v / 2, sq / 2 (RBF): the rounding of
the exponential's argument and a few operations of the map.  nrm and a grow as 1 / l, so u_K grows as 1 / l^2.

Cholesky (`u_C`).  The computed factor of any Cholesky variant satisfies |L L^T - K| <= (n + 1) eps |L||L^T|
(Higham, Accuracy and Stability, thm 10.3); the residual is evaluated in extended precision against the K that
was factored.  `u_C_from_K` is the same bound through Cauchy-Schwarz, (n + 1) eps sqrt(K_ii K_jj), for the one
situation without a reference factor (see `test_gpu_gp_edges.py`, jitter ladder).

Root inverse (`u_R`).  Substitution, column by column, leaves |L R - I| <= n eps |L||R|.  The blocked form
computes block row I of a column chunk as X_I = Rd_I S, S = -sum_{K<I} L_IK X_K, with Rd_I the INVERTED diagonal
block: L_II Rd_I = I + E_I, |E_I| <= BLOCK eps |L_II||Rd_I|, and the product Rd_I S adds BLOCK eps |Rd_I||S|.
Row I of the residual is dS + E_I S + L_II dP: the first is inside n eps |L||R|, the other two are
  2 BLOCK eps |L_II||Rd_I||S|,      S = sum_{K<I} L_IK R_K (reference values), BLOCK = 64.
It is there because multiplying by an explicit inverse is only as good as that inverse's own residual - a
substitution with L_II would not need it.  (The diagonal blocks themselves need no such term.)

alpha.  With R~ = R (I + E), |E| <= u_R, t~ = R~ y_s + dt, |dt| <= n eps |R||y_s|, alpha~ = R~^T t~ + da,
|da| <= n eps |R^T||t|, and K~ = L L^T + dC, |dC| <= u_C:
  residual  K~ alpha~ - y_s:  u_res = |L||L^T| u_R^T |alpha| + u_R |y_s| + n eps |L||R||y_s| + n eps |K||R^T||t|
                                      + u_C |alpha| + 2 eps |y_s|
  forward   alpha~ - alpha :  u_fw  = |R^T||R| ((u_K + u_C) |alpha| + u_ys) + u_R^T |R^T||t| + |R^T||R| u_R |y_s|
                                      + n eps |R^T||R||y_s| + n eps |R^T||t|
  u_ys = eps (n mean|y| / sd + (n + 2) |y_s|)   (mean and sd of n terms)
the kappa-type factor |R^T||R| >= |K^-1| is the price of the explicit inverse and of judging against the exact
alpha of the exact K.  The residual is taken against y_s formed from the implementation's OWN mean and sd.

Computed factors.  Both residual bounds hold with the COMPUTED |L| and |R| on the right.  Where K is nearly
banded (short lengthscale) exact entries of L and R far from the diagonal decay to 1e-20 and less while the
computed ones stop at the forward error of their neighbours, so the exact factors would give units that are too
small by orders of magnitude there.  Every unit therefore uses
  |L|' = |L| + |L| tril(|R| u_C |R^T|),   |R|' = |R| + |R| tril(n eps |L|'|R|)
(the first-order forward errors dL = L tril(L^-1 dK L^-T), dR = R E), which are |L|, |R| up to O(eps) relative
wherever the entries are not that small.

diag(R).  R_ii = 1 / L_ii is one division: |R_ii L_ii - 1| <= eps (`u_diag`), with the implementation's own L.

Underflow.  fl(x op y) = (x op y)(1 + d), |d| <= eps, holds in the normal range only.  A short lengthscale takes
entries of K, L and R below it (exp(-sqrt5 d) at d > 300), where sums of n products are off by up to n 2^-1074
each and the units above, which are relative, say nothing: errors up to n 2^-1022 count as none.

Normalize bounds: 4 eps max(|min|, |max|, range) is what `test_gpu_wpca_edges.py` allows; the unit `u_nb` is a
sixteenth of it, so that the common limit of 16 units is that bound.
"""
import math
from types import SimpleNamespace

import numpy as np

from wpca_reference import EPS, EXTENDED, f64, hp, hp_sqrt

BLOCK = 64
UNDERFLOW = 2.0 ** -1022          # smallest normal double
MP_MAX_N = 40                     # largest n the mpmath path is asked for
LENGTHSCALE = 0.6931471805599453  # ln 2
NOISE = 0.006737946999085467      # e^-5
GENERATORS = ("lhs", "cluster", "twins", "shifted")
HYPERS = ("default", "short", "rbf", "wide")
GRID_N = (2, 3, 16, 17, 63, 64, 65, 127, 128, 129, 192, 193, 257, 321)
GRID_N_K = (1, 5, 33)
GRID_K = (1, 2, 3, 4, 5, 8, 33, 64, 65, 128)
GRID_K_N = (65, 129)
HYPER_N = (65, 129, 193)
HYPER_K = (1, 5)
QUANTITIES = ("K", "chol", "rinv", "alpha_res", "alpha_fw", "diag", "bounds")

if EXTENDED:
    hp_exp = np.exp
else:                                                                   # pragma: no cover - not taken on x86
    import mpmath
    hp_exp = np.frompyfunc(mpmath.exp, 1, 1)


class NotPositiveDefinite(ValueError):
    pass


# ---- the grid ----------------------------------------------------------------------------------------------------
def grid_sizes():
    """(n, k) with the default hyperparameters, n descending (small problems follow large ones in a shared context)."""
    out = {(n, k) for n in GRID_N for k in GRID_N_K} | {(n, k) for n in GRID_K_N for k in GRID_K}
    return sorted(out, key=lambda t: (-t[0], -t[1]))


GRID_PARTS = ("k1", "k5", "k33", "kgrid")


def grid_part(part):
    """The grid in four parts of similar cost: the n grid at k = 1, 5, 33 and the k grid at n = 65, 129."""
    return [(n, k) for n, k in grid_sizes() if ("k%d" % k if k in GRID_N_K else "kgrid") == part]


def hyper_sizes():
    """(n, k, hyper) of the three further hyperparameter sets."""
    return [(n, k, h) for n in sorted(HYPER_N, reverse=True) for k in HYPER_K for h in HYPERS[1:]]


# ---- generators --------------------------------------------------------------------------------------------------
def make_case(gen, n, k, hyper="default", const_y=False):
    """Seeded inputs of one case.
    lhs: uniform.  cluster: the late phase of a run - three quarters of the points within 1e-3 of the range around
    one point, the others (at least two) set the range.  twins: exact duplicate pairs (i, i + 65) where n allows
    it, so that a pair sits on both sides of a tile boundary, and (i, i + 1) pairs below; n = 2 has none (its two
    points must differ for the range to exist).  shifted: columns at 1e3 +- 5e-3 times scales from 1e-6 to 1e6."""
    rng = np.random.default_rng([GENERATORS.index(gen), n, k, HYPERS.index(hyper), 4711])
    if gen == "lhs":
        Z = rng.uniform(-3.0, 3.0, size=(n, k))
    elif gen == "cluster":
        Z = rng.uniform(-3.0, 3.0, size=(n, k))
        n_cl = min((3 * n) // 4, n - 2)
        if n_cl > 0:
            centre = rng.uniform(-2.0, 2.0, size=k)
            Z[n - n_cl:] = centre + 6e-3 * rng.uniform(-0.5, 0.5, size=(n_cl, k))
    elif gen == "twins":
        Z = rng.uniform(-3.0, 3.0, size=(n, k))
        for i in range(0, n - 65, 3):
            Z[i + 65] = Z[i]
        for i in range(1, min(n, 65) - 1, 8):
            Z[i + 1] = Z[i]
    elif gen == "shifted":
        scale = np.logspace(-6.0, 6.0, k) if k > 1 else np.ones(1)
        Z = (1e3 + 5e-3 * rng.uniform(-1.0, 1.0, size=(n, k))) * scale
    else:
        raise ValueError(gen)
    y = np.full(n, 900.0) if const_y else rng.normal(size=n) * 200.0 + 900.0
    case = SimpleNamespace(gen=gen, n=n, k=k, hyper=hyper, Z=np.ascontiguousarray(Z), y=y, lengthscale=LENGTHSCALE,
                           noise=NOISE, kernel="matern", norm_bounds=None,
                           id="%s-n%d-k%d-%s%s" % (gen, n, k, hyper, "-consty" if const_y else ""))
    if hyper == "short":
        case.lengthscale, case.noise = 0.05, 1e-6
    elif hyper == "rbf":
        case.lengthscale, case.noise, case.kernel = 3.0, 1e-4, "rbf"
    elif hyper == "wide":
        zmin, zmax = Z.min(axis=0), Z.max(axis=0)
        case.norm_bounds = np.vstack([zmin - 0.5 * (zmax - zmin), zmax + (zmax - zmin)])
    return case


def jitter_cases():
    """Inputs of the jitter ladder, all with noise = 0: K is singular up to rounding."""
    out = []
    Z = np.tile(np.array([[0.1, 0.2]]), (40, 1))
    Z[::2] += 0.5
    out.append(("twins40", Z, np.arange(40.0)))
    rng = np.random.default_rng(130)
    Z = rng.uniform(-1.0, 1.0, size=(130, 3))
    Z[65:] = Z[:65]                                     # every pair (i, i + 65): across the tile boundary
    out.append(("twins130", Z, rng.normal(size=130) * 200.0 + 900.0))
    Z = rng.uniform(-1.0, 1.0, size=(96, 3))
    Z[1::2] = Z[0::2] + 1e-9
    out.append(("near96", Z, rng.normal(size=96) * 200.0 + 900.0))
    return [SimpleNamespace(id=i, Z=np.ascontiguousarray(z), y=y, n=z.shape[0], k=z.shape[1], lengthscale=LENGTHSCALE,
                            noise=0.0, kernel="matern", norm_bounds=None, gen="twins") for i, z, y in out]


# ---- extended-precision linear algebra ---------------------------------------------------------------------------
def hp_zeros(shape):
    return hp(np.zeros(shape))


def hp_cholesky(A):
    n = A.shape[0]
    L = hp_zeros((n, n))
    for j in range(n):
        s = A[j, j] - (L[j, :j] * L[j, :j]).sum() if j else A[j, j]
        if not s > 0:
            raise NotPositiveDefinite("pivot %d is %r" % (j + 1, float(s)))
        L[j, j] = hp_sqrt(s)
        if j + 1 < n:
            L[j + 1:, j] = ((A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) if j else A[j + 1:, j]) / L[j, j]
    return L


def hp_lower_inverse(L):
    n = L.shape[0]
    R = hp_zeros((n, n))
    for i in range(n):
        R[i, i] = 1 / L[i, i]
        if i:
            R[i, :i] = -(L[i, :i] @ R[:i, :i]) / L[i, i]
    return R


# ---- the reference -----------------------------------------------------------------------------------------------
def dsq_bound(A, ZN, delta, ls):
    """`dsq` of the module docstring (n x n) and the `e` it is built from (n x k), for the norm + GEMM form of the
    squared distance: A the centred, scaled points, ZN the normalised ones (both rounded to fp64), delta the
    per-column scale error, ls the lengthscale.  `mll_reference` bounds the likelihood kernels' distances with it:
    they rebuild the Gram kernel's."""
    n, k = A.shape
    e = EPS * (np.abs(ZN) / ls + np.abs(A))
    P, Q = np.zeros((n, n)), np.zeros((n, n))
    for c in range(k):
        D = np.abs(A[:, c, None] - A[None, :, c])
        P += D * (e[:, c, None] + e[None, :, c])
        Q += delta[c] * D * D
    nrm = (A * A).sum(axis=1)
    dsq = 2.0 * P + 2.0 * Q + (k + 2) * EPS * (nrm[:, None] + nrm[None, :] + 2.0 * (np.abs(A) @ np.abs(A).T))
    return dsq, e


def gram_reference(case):
    """Bounds, K and y_s of a case in extended precision with `u_K`, `u_ys`, `u_nb`."""
    Z = np.asarray(case.Z, dtype=np.float64)
    n, k = Z.shape
    if not EXTENDED and n > MP_MAX_N:
        return SimpleNamespace(skip="np.longdouble is a plain double here and n = %d is beyond the mpmath path" % n)
    ls, s2 = float(case.lengthscale), float(case.noise)
    zmin, zmax = Z.min(axis=0), Z.max(axis=0)
    if case.norm_bounds is None:
        rng = hp(zmax) - hp(zmin)
        lo, hi = hp(zmin) - hp(0.1) * rng, hp(zmax) + hp(0.1) * rng
        delta = EPS * (0.5 * (np.abs(f64(lo)) + np.abs(f64(hi))) / f64(hi - lo) + 3.0) if np.all(zmax > zmin) else None
    else:
        lo, hi = hp(case.norm_bounds[0]), hp(case.norm_bounds[1])
        delta = np.full(k, 3.0 * EPS)
    with np.errstate(all="ignore"):
        zn = (hp(Z) - lo) / (hi - lo)
        a = (zn - zn.sum(axis=0) / n) / hp(ls)
        sq = hp_zeros((n, n))
        for c in range(k):
            diff = a[:, c, None] - a[None, :, c]
            sq = sq + diff * diff
        if case.kernel == "rbf":
            v = hp_exp(-sq / 2)
        else:
            s5, d = hp_sqrt(hp(5.0)), hp_sqrt(sq)
            v = (1 + s5 * d + hp(5.0) / hp(3.0) * sq) * hp_exp(-s5 * d)
    K = v + hp(s2) * hp(np.eye(n))
    yh = hp(case.y)
    ym = yh.sum() / n
    sd = hp_sqrt(((yh - ym) ** 2).sum() / (n - 1))
    if not sd >= 1e-8:
        sd = hp(1.0)
    ys = (yh - ym) / sd
    ref = SimpleNamespace(skip=None, n=n, k=k, lo=lo, hi=hi, K=K, ys=ys, ym=ym, sd=sd, u_K=None,
                          u_nb=0.25 * EPS * np.maximum(np.maximum(np.abs(zmin), np.abs(zmax)), zmax - zmin),
                          u_ys=EPS * (n * np.abs(case.y).mean() / float(sd) + (n + 2) * np.abs(f64(ys))))
    if delta is None:                                   # a column without a range: K is NaN, there is nothing to bound
        return ref
    A, ZN, V, SQ = f64(a), f64(zn), f64(v), f64(sq)
    dsq, _ = dsq_bound(A, ZN, delta, ls)
    sq_lo = np.maximum(SQ - dsq, 0.0)
    if case.kernel == "rbf":
        u_K = 0.5 * np.exp(-0.5 * sq_lo) * dsq + EPS * np.abs(V) * (4.0 + 0.5 * SQ)
    else:
        s5 = math.sqrt(5.0)
        d_lo = np.sqrt(sq_lo)
        u_K = 5.0 / 6.0 * (1.0 + s5 * d_lo) * np.exp(-s5 * d_lo) * dsq + EPS * np.abs(V) * (4.0 + s5 * np.sqrt(SQ))
    np.fill_diagonal(u_K, 2.0 * EPS * (1.0 + s2))
    ref.u_K = u_K
    return ref


def _blocks(n):
    return [(b, min(b + BLOCK, n)) for b in range(0, n, BLOCK)]


def factor_reference(K, ys, u_K=None, u_ys=None):
    """L, R, t, alpha of K (extended precision) with `u_C`, `u_R`, `u_res`, `u_fw`; NotPositiveDefinite if K is not."""
    n = K.shape[0]
    L = hp_cholesky(K)
    R = hp_lower_inverse(L)
    t = R @ ys
    alpha = R.T @ t
    aL, aR, aK = np.abs(f64(L)), np.abs(f64(R)), np.abs(f64(K))
    # the computed factors, not the exact ones, stand in the bounds: add what they may differ by
    aL = aL + aL @ np.tril(aR @ ((n + 1) * EPS * (aL @ aL.T)) @ aR.T)
    aR = aR + aR @ np.tril(n * EPS * (aL @ aR))
    ya, ta, al = np.abs(f64(ys)), np.abs(f64(t)), np.abs(f64(alpha))
    u_C = (n + 1) * EPS * (aL @ aL.T)
    u_R = n * EPS * (aL @ aR)
    Loff = f64(L).copy()
    for b0, b1 in _blocks(n):
        Loff[b0:b1, b0:] = 0.0
    S = np.abs(Loff @ f64(R))
    for b0, b1 in _blocks(n):
        u_R[b0:b1] += 2.0 * BLOCK * EPS * ((aL[b0:b1, b0:b1] @ aR[b0:b1, b0:b1]) @ S[b0:b1])
    u_R = np.tril(u_R)
    u_res = (aL @ (aL.T @ (u_R.T @ al)) + u_R @ ya + n * EPS * (aL @ (aR @ ya)) + n * EPS * (aK @ (aR.T @ ta))
             + u_C @ al + 2.0 * EPS * ya)
    u_K = np.zeros((n, n)) if u_K is None else u_K
    u_ys = np.zeros(n) if u_ys is None else u_ys

    def kinv(vec):
        return aR.T @ (aR @ vec)

    u_fw = (kinv((u_K + u_C) @ al + u_ys) + u_R.T @ (aR.T @ ta) + kinv(u_R @ ya) + n * EPS * kinv(ya)
            + n * EPS * (aR.T @ ta))
    return SimpleNamespace(n=n, K=K, ys=ys, L=L, R=R, t=t, alpha=alpha, u_C=u_C, u_R=u_R, u_res=u_res, u_fw=u_fw,
                           u_diag=EPS)


def u_C_from_K(K):
    """(n + 1) eps sqrt(K_ii K_jj) >= (n + 1) eps (|L||L^T|)_ij for the exact factor (Cauchy-Schwarz on its rows)."""
    dg = np.sqrt(np.abs(np.diag(f64(K))))
    return (K.shape[0] + 1) * EPS * np.outer(dg, dg)


def reference(case):
    """gram_reference + factor_reference of one case in one namespace (`skip` set where there is no reference)."""
    g = gram_reference(case)
    if g.skip:
        return g
    f = factor_reference(g.K, g.ys, g.u_K, g.u_ys)
    g.__dict__.update({key: val for key, val in f.__dict__.items() if key not in ("K", "ys", "n")})
    return g


# ---- judging an implementation ----------------------------------------------------------------------------------
def _ratio(err, unit):
    """max err / unit; an error where the unit is zero counts as infinite, NaN anywhere as infinite.  Errors up to
    n UNDERFLOW count as none (see the module docstring)."""
    err, unit = np.abs(f64(err)), np.asarray(unit, dtype=np.float64)
    if not np.all(np.isfinite(err)):
        return float("inf")
    err = np.where(err <= UNDERFLOW * max(err.shape), 0.0, err)
    if np.any(err[unit == 0.0] != 0.0):
        return float("inf")
    pos = unit > 0.0
    return float((err[pos] / unit[pos]).max()) if pos.any() else 0.0


def judge_factor(fref, K, L, R, alpha, y, y_mean, y_std, K_factored=None):
    """Ratios of an implementation's L, R, alpha to the units of `fref`.  K: the matrix it factored (its own Gram
    matrix, plus jitter where it added some: `K_factored`)."""
    n = fref.n
    Kf = hp(K if K_factored is None else K_factored)
    Lh, Rh, ah = hp(L), hp(R), hp(alpha)
    out = SimpleNamespace()
    out.chol = _ratio(Lh @ Lh.T - Kf, fref.u_C)
    out.rinv = _ratio(np.tril(f64(Lh @ Rh - hp(np.eye(n)))), fref.u_R)
    ys_own = (hp(y) - hp(y_mean)) / hp(y_std)
    out.alpha_res = _ratio(Kf @ ah - ys_own, fref.u_res)
    out.alpha_fw = _ratio(ah - fref.alpha, fref.u_fw)
    out.diag = _ratio(hp(np.diag(R)) * hp(np.diag(L)) - 1, np.full(n, fref.u_diag))
    out.upper_zero = bool(np.all(np.triu(L, 1) == 0.0) and np.all(np.triu(R, 1) == 0.0))
    out.diag_positive = bool(np.all(np.diag(L) > 0.0))
    return out


def judge(ref, K, L, R, alpha, y, y_mean, y_std, norm_bounds):
    """judge_factor plus K against the reference K, its symmetry and the Normalize bounds."""
    out = judge_factor(ref, K, L, R, alpha, y, y_mean, y_std)
    out.K = _ratio(hp(K) - ref.K, ref.u_K)
    out.symmetric = bool(np.array_equal(K, K.T))
    nb = np.asarray(norm_bounds, dtype=np.float64)
    out.bounds = max(_ratio(hp(nb[0]) - ref.lo, ref.u_nb), _ratio(hp(nb[1]) - ref.hi, ref.u_nb))
    return out


FLAGS = ("upper_zero", "diag_positive", "symmetric")
RUNGS = (0.0, 1e-8, 1e-7, 1e-6)


def judge_ladder(case, K, L, R, alpha, y_mean, y_std):
    """An accepted factorisation of K + j I with j one of psd_safe_cholesky's rungs.  `seen`: the median of
    diag(L L^T) - diag(K); `rung`: the nearest rung; `ratios`: the Cholesky residual against K + rung I, the root
    inverse and alpha in the units of the reference factorisation of K + rung I.  At rung 0 of a K that is singular
    to working precision there is no such reference and no first-order unit means anything for R and alpha: only the
    Cholesky residual is judged, in `u_C_from_K`."""
    n = K.shape[0]
    Lh = hp(L)
    out = SimpleNamespace()
    out.finite = bool(np.all(np.isfinite(L)) and np.all(np.isfinite(R)) and np.all(np.isfinite(alpha)))
    out.seen = float(np.median(f64((Lh * Lh).sum(axis=1) - hp(np.diag(K))))) if out.finite else float("nan")
    out.rung = min(RUNGS, key=lambda r: abs(out.seen - r)) if out.finite else float("nan")
    out.ratios, out.flags_ok = {}, out.finite
    if not out.finite:
        return out
    Kf = K.copy()
    Kf[np.diag_indices(n)] += out.rung
    if out.rung == 0.0:
        out.ratios["chol"] = _ratio(Lh @ Lh.T - hp(Kf), u_C_from_K(Kf))
        return out
    ys = (hp(case.y) - hp(y_mean)) / hp(y_std)
    fref = factor_reference(hp(Kf), ys)
    j = judge_factor(fref, K, L, R, alpha, case.y, y_mean, y_std, K_factored=Kf)
    out.ratios = {q: getattr(j, q) for q in ("chol", "rinv", "alpha_res", "alpha_fw", "diag")}
    out.flags_ok = bool(j.upper_zero and j.diag_positive)
    return out


# ---- the documented algorithm in plain fp64 ----------------------------------------------------------------------
def blocked_cholesky(K, drop=None):
    """Left-looking Cholesky in 64-wide panels, fp64.  drop = (I, J, p): the product of panel p is left out of the
    update of block (I, J) - a deliberately wrong variant."""
    from scipy.linalg import solve_triangular
    n = K.shape[0]
    A = np.tril(K).copy()
    bl = _blocks(n)
    for J, (j0, j1) in enumerate(bl):
        for I in range(J, len(bl)):
            i0, i1 = bl[I]
            for p in range(J):
                if drop == (I, J, p):
                    continue
                p0, p1 = bl[p]
                A[i0:i1, j0:j1] -= A[i0:i1, p0:p1] @ A[j0:j1, p0:p1].T
        D = np.tril(A[j0:j1, j0:j1])
        A[j0:j1, j0:j1] = np.linalg.cholesky(D + np.tril(D, -1).T)
        if j1 < n:
            A[j1:, j0:j1] = solve_triangular(A[j0:j1, j0:j1], A[j1:, j0:j1].T, lower=True).T
    return np.tril(A)


def restate(case, coef53=5.0 / 3.0, matvec_strict=False, drop=None, jitter=0.0):
    """numpy fp64 restatement of the chain: norms + dot product for the distance, np.linalg.cholesky,
    scipy.linalg.solve_triangular for R, two mat-vecs for alpha.  The keyword arguments switch on one wrong variant
    each: the 5/3 of the Matern map (pass a float32), `j < i` in t = R y_s, one dropped panel product (blocked_cholesky)."""
    from scipy.linalg import solve_triangular
    Z, y = np.asarray(case.Z, dtype=np.float64), np.asarray(case.y, dtype=np.float64)
    n, k = Z.shape
    if case.norm_bounds is None:
        zmin, zmax = Z.min(axis=0), Z.max(axis=0)
        rng = zmax - zmin
        lo, hi = zmin - 0.1 * rng, zmax + 0.1 * rng
    else:
        lo, hi = np.asarray(case.norm_bounds[0], dtype=np.float64), np.asarray(case.norm_bounds[1], dtype=np.float64)
    with np.errstate(all="ignore"):
        zn = (Z - lo) / (hi - lo)
        a = (zn - (Z.sum(axis=0) / n - lo) / (hi - lo)) * (1.0 / case.lengthscale)
        nrm = (a * a).sum(axis=1)
        sq = (nrm[:, None] + nrm[None, :]) - 2.0 * (a @ a.T)
        np.fill_diagonal(sq, 0.0)
        sq = np.where(sq < 0.0, 0.0, sq)
        if case.kernel == "rbf":
            K = np.exp(-0.5 * sq)
        else:
            d = np.sqrt(np.where(sq < 1e-30, 1e-30, sq))
            K = ((math.sqrt(5.0) * d + 1.0) + float(coef53) * (d * d)) * np.exp(-math.sqrt(5.0) * d)
    K[np.diag_indices(n)] += case.noise
    ym = y.sum() / n
    sd = math.sqrt(((y - ym) ** 2).sum() / (n - 1))
    if not sd >= 1e-8:
        sd = 1.0
    ys = (y - ym) / sd
    Kf = K.copy()
    Kf[np.diag_indices(n)] += jitter
    L = blocked_cholesky(Kf, drop) if drop is not None else np.linalg.cholesky(Kf)
    R = np.tril(solve_triangular(L, np.eye(n), lower=True))
    t = (np.tril(R, -1) if matvec_strict else R) @ ys
    alpha = R.T @ t
    return SimpleNamespace(K=K, K_factored=Kf, L=L, R=R, alpha=alpha, y_mean=ym, y_std=sd, norm_bounds=np.vstack([lo, hi]))


class Worst:
    """Worst ratio per quantity and generator, for the table the tests print."""

    def __init__(self):
        self.w = {}

    def add(self, gen, quantity, value, case_id):
        key = (gen, quantity)
        if key not in self.w or not value <= self.w[key][0]:
            self.w[key] = (float(value), case_id)

    def table(self, title):
        qs = [q for q in QUANTITIES if any(key[1] == q for key in self.w)]
        lines = [title, "%-10s" % "generator" + "".join("%11s" % q for q in qs)]
        for g in GENERATORS:
            if any((g, q) in self.w for q in qs):
                lines.append("%-10s" % g + "".join("%11.3g" % self.w.get((g, q), (float("nan"),))[0] for q in qs))
        for q in qs:
            v, cid = max((self.w[(g, q)] for g in GENERATORS if (g, q) in self.w), key=lambda t: t[0])
            lines.append("  worst %-10s %10.3g  %s" % (q, v, cid))
        return "\n".join(lines)
