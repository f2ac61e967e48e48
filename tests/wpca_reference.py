"""Extended-precision reference of the rank-weighted PCA and the error units its results are judged in.

No tests here: `test_wpca_reference_cpu.py` proves the reference and its units on the sklearn path,
`test_gpu_wpca_edges.py` judges the HIP kernels of `kernels_wpca.hip` by them.

Arithmetic: `np.longdouble` where it carries a 64-bit mantissa (x86).  Where it is a plain double the same
formulas run on object arrays of `mpmath.mpf` (30 digits), on the small cases only; `reference()` then marks the
large ones with a `skip` reason.

Error units (first-order analysis of ANY fp64 implementation, eps = 2**-52; none of them comes from a run of
the code under test):
  dW        = eps ((2|X| + 2|mu|) sqrt(w) + 4|W|)             centring + weighting + noise, per element
  T         = d eps ||C||_2 + 2 ||Wc||_F ||dW||_F / (n - 1)   eigen-solver backward error + conditioning of C
  u_dmean_j = n eps mean_i |X_ij|
  u_pmean_j = mean_i dW_ij + n eps mean_i |W_ij|
  u_orth    = d eps
"""
import math
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -52
EXTENDED = bool(np.finfo(np.longdouble).eps < 2.2e-16)
MP_WORK_LIMIT = 2.0e5            # n d^2 above which the mpmath path is not attempted

GENERATORS = ("lhs", "cluster", "twin", "shifted")
GRID_D = (1, 2, 3, 5, 7, 10, 16, 17, 20, 33, 40, 63, 64, 65, 100, 127, 128)


def grid_n(d):
    """n of the grid for this d, n >= 2, repeats (d = n, d + 1 = n) once."""
    out = []
    for n in (2, 3, 5, d, d + 1, 31, 120, 257, 450, 513, 1050):
        if n >= 2 and n not in out:
            out.append(n)
    return out


def grid_cases():
    """Every (generator, d, n) of the grid: 186 (d, n) combinations per generator, 181 of them distinct."""
    return [(g, d, n) for g in GENERATORS for d in GRID_D for n in grid_n(d)]


# ---- extended-precision plumbing ---------------------------------------------------------------------------------
if EXTENDED:
    def hp(a):
        return np.asarray(a, dtype=np.longdouble)

    hp_sqrt, hp_log = np.sqrt, np.log
else:                                                                   # pragma: no cover - not taken on x86
    import mpmath
    mpmath.mp.dps = 30
    _mpf = np.frompyfunc(lambda v: mpmath.mpf(float(v)) if not isinstance(v, mpmath.mpf) else v, 1, 1)
    _mps = np.frompyfunc(mpmath.sqrt, 1, 1)
    _mpl = np.frompyfunc(mpmath.log, 1, 1)

    def hp(a):
        return _mpf(np.asarray(a, dtype=object))

    def hp_sqrt(a):
        return _mps(a)

    def hp_log(a):
        return _mpl(a)


def f64(a):
    return np.asarray(a).astype(np.float64)


def _mean0(a, exact_of=None):
    """Column means; on the mpmath path the means of fp64 data are taken with math.fsum."""
    n = a.shape[0]
    if not EXTENDED and exact_of is not None:
        return hp([math.fsum(exact_of[:, j]) for j in range(a.shape[1])]) / n
    return a.sum(axis=0) / n


def stable_ranks(f, maximize=False):
    """1-based rank of each f, best first, ties by index (what k_rank promises)."""
    f = np.asarray(f, dtype=np.float64)
    key = -f if maximize else f
    return np.argsort(np.argsort(key, kind="stable"), kind="stable") + 1


# ---- generators --------------------------------------------------------------------------------------------------
def _orthogonal(rng, d):
    q, r = np.linalg.qr(rng.normal(size=(d, d)))
    return q * np.sign(np.diag(r))


def make_case(gen, d, n, salt=0):
    """Seeded inputs of one case: X (n x d), ranks (from a seeded normal f), f, noise N(0, 1e-8) as in the algorithm."""
    rng = np.random.default_rng([GENERATORS.index(gen), d, n, salt, 20240])
    if gen == "lhs":
        X = rng.uniform(-5.0, 5.0, size=(n, d))
    elif gen in ("cluster", "twin"):
        if gen == "cluster":
            sd = np.logspace(0.0, -6.0, d)
        else:
            sd = np.repeat(np.logspace(0.0, -3.0, (d + 1) // 2), 2)[:d]
        X = (rng.normal(size=(n, d)) * sd) @ _orthogonal(rng, d) + rng.uniform(-3.0, 3.0, size=d)
    elif gen == "shifted":
        X = 1e3 + 1e-3 * rng.uniform(-5.0, 5.0, size=(n, d))
    else:
        raise ValueError(gen)
    f = rng.normal(size=n)
    noise = rng.normal(0.0, 1e-8, size=(n, d))
    return SimpleNamespace(gen=gen, d=d, n=n, X=np.ascontiguousarray(X), f=f, ranks=stable_ranks(f), noise=noise,
                           id="%s-d%d-n%d" % (gen, d, n) + ("-s%d" % salt if salt else ""))


# ---- the reference -----------------------------------------------------------------------------------------------
def reference(X, ranks, noise):
    """Weights (ln n - ln r) / sum, mu, W = (X - mu) sqrt(w) + noise, mw, Wc, C = Wc^T Wc / (n - 1) in extended
    precision, and the error units.  `rho`: the eigenvalues of C (fp64 LAPACK on the rounded C: absolute error
    d eps ||C||, i.e. below T), descending, the first min(n, d) as sklearn keeps them."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    if not EXTENDED and float(n) * d * d > MP_WORK_LIMIT:
        return SimpleNamespace(n=n, d=d, skip="np.longdouble is a plain double here and n d^2 = %d is beyond the "
                                              "mpmath path" % (n * d * d))
    Xh = hp(X)
    pre = hp_log(hp(float(n))) - hp_log(hp(np.asarray(ranks, dtype=np.float64)))
    w = pre / pre.sum()
    mu = _mean0(Xh, exact_of=X)
    W = (Xh - mu) * hp_sqrt(w)[:, None]
    if noise is not None:
        W = W + hp(noise)
    mw = _mean0(W)
    Wc = W - mw
    C = (Wc.T @ Wc) / (n - 1)
    C = (C + C.T) / 2

    aX, amu, aW, w64, C64 = np.abs(X), np.abs(f64(mu)), np.abs(f64(W)), f64(w), f64(C)
    dW = EPS * ((2.0 * aX + 2.0 * amu) * np.sqrt(w64)[:, None] + 4.0 * aW)
    T = d * EPS * np.linalg.norm(C64, 2) + 2.0 * np.linalg.norm(f64(Wc)) * np.linalg.norm(dW) / (n - 1)
    rc = min(n, d)
    lam = np.linalg.eigvalsh(C64)[::-1]
    rho = np.maximum(lam, 0.0)[:rc]
    return SimpleNamespace(n=n, d=d, skip=None, w=w, mu=mu, W=W, mw=mw, Wc=Wc, C=C, dW=dW, T=float(T),
                           u_dmean=n * EPS * aX.mean(axis=0), u_pmean=dW.mean(axis=0) + n * EPS * aW.mean(axis=0),
                           u_orth=d * EPS, rho=rho, rho_all=np.maximum(lam, 0.0), trC=float(np.trace(C64)))


def cumulative_margin(rho, var_threshold=0.95):
    """Distance of the nearest cumulative rho / sum(rho) to the threshold (the selection step is exact when it is
    far above the rounding of the ratios)."""
    rho = np.asarray(rho, dtype=np.float64)
    return float(np.abs(np.cumsum(rho / rho.sum()) - var_threshold).min())


def gaps(ref):
    """Distance from rho_r to the nearest other eigenvalue of C, for the rows sklearn keeps."""
    lam = ref.rho_all
    out = np.empty(len(ref.rho))
    for r in range(len(ref.rho)):
        other = np.delete(lam, r)
        out[r] = np.abs(other - lam[r]).min() if other.size else np.inf
    return out


def invariants(C, T, comps, evr):
    """Properties of an eigen-decomposition (components as rows, explained-variance ratios) that need no comparison
    vector by vector, as multiples of the units: so paired and near-degenerate eigenvalues can be judged."""
    comps = np.asarray(comps, dtype=np.float64)
    evr = np.asarray(evr, dtype=np.float64)
    rc, d = comps.shape
    u_orth = d * EPS
    V = hp(comps)
    CV = V @ C                                              # rows (C v_r)^T: C is symmetric
    rho = (CV * V).sum(axis=1)
    trC = sum(C[j, j] for j in range(d))
    rho64 = f64(rho)
    live = rho64 > 1e3 * T
    res = CV - rho[:, None] * V
    resn = np.sqrt(f64((res * res).sum(axis=1)))
    out = SimpleNamespace(rho=rho64, live=live, n_live=int(live.sum()))
    out.residual = float((resn[live] / T).max()) if live.any() else 0.0
    Vl = V[live]
    gram = f64(Vl @ Vl.T - hp(np.eye(Vl.shape[0])))
    out.orth = float(np.abs(gram).max() / u_orth) if live.any() else 0.0
    dev = np.abs(f64(hp(evr) - rho / trC))
    out.evr = float((dev[live] / (T / float(trC))).max()) if live.any() else 0.0
    out.evr_monotone = bool(np.all(np.diff(evr) <= 0.0))
    sign_ok = True
    for r in np.nonzero(live)[0]:
        a = np.abs(comps[r])
        o = np.argsort(a)
        if d == 1 or a[o[-1]] - a[o[-2]] > 1e-6 * a[o[-1]]:
            sign_ok = sign_ok and comps[r, o[-1]] > 0.0
    out.sign_ok = bool(sign_ok)
    dead = comps[~live]
    out.dead_ok = bool(np.all(np.isfinite(dead)) and
                       (dead.size == 0 or np.sqrt((dead * dead).sum(axis=1)).max() <= 1.0 + 16.0 * u_orth))
    out.finite = bool(np.all(np.isfinite(comps)) and np.all(np.isfinite(evr)))
    return out


QUANTITIES = ("residual", "orth", "evr", "data_mean", "pca_mean")


def judge(ref, data_mean, pca_mean, comps, evr):
    """invariants() plus the two means against the reference, everything in units."""
    inv = invariants(ref.C, ref.T, comps, evr)
    inv.data_mean = float((np.abs(f64(hp(data_mean) - ref.mu)) / ref.u_dmean).max())
    inv.pca_mean = float((np.abs(f64(hp(pca_mean) - ref.mw)) / ref.u_pmean).max())
    return inv


def project_reference(X, data_mean, pca_mean, ck):
    """Z = (X - mu) Ck^T - mw Ck^T from the GIVEN means and components (isolates the projection), and its unit
    (d + 2) eps sum_j (|x_j - mu_j| + |mw_j|) |c_j| per element."""
    d = X.shape[1]
    xc = hp(X) - hp(data_mean)
    ckh = hp(ck)
    Z = xc @ ckh.T - (hp(pca_mean)[None, :] @ ckh.T)
    unit = (d + 2) * EPS * ((np.abs(f64(xc)) + np.abs(pca_mean)[None, :]) @ np.abs(ck).T)
    return Z, unit


def inverse_reference(z, data_mean, pca_mean, ck):
    """x = z Ck + mw + mu and its unit (k + 2) eps (sum_c |z_c c_cj| + |mw_j| + |mu_j|)."""
    k = ck.shape[0]
    x = hp(z)[None, :] @ hp(ck) + hp(pca_mean) + hp(data_mean)
    unit = (k + 2) * EPS * (np.abs(z) @ np.abs(ck) + np.abs(pca_mean) + np.abs(data_mean))
    return x.ravel(), unit


class Worst:
    """Worst ratio per quantity and generator, for the table the tests print."""

    def __init__(self):
        self.w = {}

    def add(self, gen, quantity, value, case_id):
        key = (gen, quantity)
        if key not in self.w or value > self.w[key][0]:
            self.w[key] = (float(value), case_id)

    def table(self, title):
        qs = sorted({q for _, q in self.w})
        lines = [title, "%-10s" % "generator" + "".join("%12s" % q for q in qs)]
        for g in GENERATORS:
            if any((g, q) in self.w for q in qs):
                lines.append("%-10s" % g + "".join("%12.3g" % self.w.get((g, q), (float("nan"),))[0] for q in qs))
        for q in qs:
            v, cid = max((self.w[(g, q)] for g in GENERATORS if (g, q) in self.w), key=lambda t: t[0])
            lines.append("  worst %-10s %10.3g  %s" % (q, v, cid))
        return "\n".join(lines)
