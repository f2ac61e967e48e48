"""Extended-precision reference of the GP fit's loss and gradient at a conditioned state, and their error units.

No tests here: `test_mll_reference_cpu.py` proves the reference and its units on a plain numpy restatement,
`test_gpu_mll_edges.py` judges `k_mll_grad<false>`, `k_mll_grad<true>`, `k_mll_finish<>` (csrc/kernels_fit.hip) and
`mll_assemble` (csrc/host_side.h) by them.  Nothing of `test_gp_fit_cpu`, `ard_reference` or the library is called.

The reference starts from a state conditioned at theta and takes its fp64 arrays as exact, as `acq_reference` does
for the acquisition: {L, R, alpha, y_mean (= m' = m + s c), y_std, norm_bounds} as `pcabo_get_gp_state` returns them
(the raw n x n blocks), with Z, y and theta = (s2, c, rho) or (s2, c, rho_1 .. rho_k).  The conditioning itself is
judged by `gp_reference`, so none of its kappa-type factors enter here.

  ys_i = (y_i - m') / s
  zn   = (Z - lo) / (hi - lo)                      the state's bounds; ARD: the folded ones, hi' = lo + (hi - lo) l_c
  a    = zn / l                                    scalar: l = softplus(rho), torch's threshold 20; ARD: l = 1
  sq_ij = sum_c (a_ic - a_jc)^2                    taken DIRECTLY, never norms + dot product;  d = sqrt(sq)
  h0 = sum_i log L_ii   h1 = ys . alpha   h2 = sum alpha   h3 = alpha . alpha   h4 = tr Kinv,  Kinv = R^T R
  W = alpha alpha^T - Kinv
  scalar:  S   = sum_{i != j} W_ij w_ij,             w = (5/3) sq (1 + sqrt5 d) exp(-sqrt5 d)
  ARD:     S_c = sum_{i != j} W_ij g_ij D_ijc^2,     g = (5/3) (1 + sqrt5 d) exp(-sqrt5 d),  D_ijc = a_ic - a_jc
  lnz = log s2, u = lnz + 4                        LogNormal(-4, 1) prior on s2
  loss      = (h1 / 2 + h0 + n log(2 pi) / 2 + lnz + log(2 pi) / 2 + u^2 / 2) / n
  grad[s2]  = -((h3 - h4) / 2 - (1 + u) / s2) / n
  grad[c]   = -h2 / n
  grad[rho] = -(S / 2) (dl / drho) / l / n         dl / drho = 1 for rho > 20 (l = rho there), the sigmoid otherwise -
                                                   in BOTH forms: it is the derivative of the softplus the loss uses
in `np.longdouble` (where it is a plain double the same formulas run on mpmath objects, n <= gp_reference.MP_MAX_N).
`sums(..., arith=mp_arith(40))` evaluates the same text with 40 digits; `loss_from_scratch` is the loss with no state
at all (Normalize, Gram, Cholesky in extended precision), which the CPU test differentiates numerically to prove
that the formulas above are its gradient.

Error units: first-order bounds of what ANY fp64 implementation of this chain commits (eps = 2^-52), computed from
reference quantities only.  |.| elementwise, sums over i != j unless said otherwise.

dsq_ij.  The kernels rebuild the Gram kernel's distance from the centred a and their norms, so the bound is
`gp_reference.dsq_bound` (the norm + GEMM form: e_ic, delta_c and the (k + 2) eps (nrm_i + nrm_j + 2 sum |a_ic a_jc|)
term).  The bounds are the state's, exact: delta_c = 3 eps (the division, 1 / l, the product).  In the scalar form
l itself is the host's log1p(exp(rho)) rounded once more on its way into 1 / l - two more relative eps on every
column alike - so delta_c = 5 eps there.
Weight (scalar), dw/dsq = (5/3) exp(-sqrt5 d) (1 + sqrt5 d - 5/2 sq), which changes sign, so its size is taken at both
ends and the middle of the interval the computed sq lies in:
  dw = max_{sq - dsq (>= 0), sq, sq + dsq} |dw/dsq| dsq + eps |w| (6 + sqrt5 d)
(6: the products and the sum of the map; sqrt5 d: the rounding of the exponential's argument).
ARD, dg/dsq = -(25/6) exp(-sqrt5 d):
  dg = (25/6) exp(-sqrt5 d_lo) dsq + eps |g| (5 + sqrt5 d),      d_lo = sqrt(max(sq - dsq, 0))
  d(D_c^2) = 2 |D_c| (e_ic + e_jc) + 2 (delta_c + eps) D_c^2     (the direct square)
Inverse and W:  dKinv_ij = (n + 2) eps sum_p |R_pi R_pj|,  d(alpha_i alpha_j) = eps |alpha_i alpha_j|, and one
eps |W_ij| for the subtraction:  dW = dKinv + 2 eps |alpha_i alpha_j| + eps |W|.
  uS   = sum (|W| dw + |w| dW) + (2n + 4) eps sum |W w|
  uS_c = sum (|W| (dg D_c^2 + |g| d(D_c^2)) + |g| D_c^2 dW) + (2n + 4) eps sum |W g| D_c^2
(the last term: a sum of n (n - 1) terms in any order of depth <= 2n + 4).
  u0 = (n + 3) eps sum |log L_ii|
  u1 = (n + 2) eps sum |ys_i alpha_i| + sum |alpha_i| u_ys_i,   u_ys_i = eps ((|y_i| + |m'|) / s + 3 |ys_i| + |c|)
  u2 = (n + 2) eps sum |alpha_i|      u3 = (n + 2) eps h3      u4 = (2n + 4) eps h4
Loss and gradient: the product rule through the formulas above, plus HOST = 8 eps at the size of the terms for the
host's arithmetic (one log, one log1p(exp) and one sigmoid of libm at an ulp or two each, the rounded constant
log(2 pi), and chains of at most six operations whose partial sums stay below the sum of the absolute terms):
  u_loss      = (u0 + u1 / 2) / n + HOST (|h0| + |h1| / 2 + n log(2 pi) / 2 + |lnz| + log(2 pi) / 2 + u^2 / 2 + |u lnz|) / n
  u_grad[s2]  = ((u3 + u4) / 2 + HOST ((h3 + h4) / 2 + (1 + |u| + |lnz|) / s2)) / n
  u_grad[c]   = (u2 + HOST |h2|) / n
  u_grad[rho] = (uS / 2 + HOST |S| / 2) (dl / drho) / l / n
Underflow, as in `gp_reference`: an error up to n 2^-1022 counts as none.

What the units can and cannot see (`test_mll_reference_cpu.py::test_units_notice_wrong_variants` prints the
margins).  uS is a sum of ABSOLUTE terms |W_ij| dw_ij: where W w changes sign and S is a small remainder, uS / |S|
is large, and a RELATIVE defect of S, such as the float 5/3 (4e-8) or the sigmoid slope (1.25e-9), shows only where
S keeps a good part of sum |W w| - small uniform states, and there by orders of magnitude.  Each variant is
therefore asserted on the state named beside it.  The ARD square expanded as a_i^2 + a_j^2 - 2 a_i a_j is the
sharpest example.  Its error per pair is a few eps a_ic^2 |W g|, where the direct square's unit is 2 |D_c| (e_ic + e_jc)
|W g|: far above it on close pairs (|D_c| << |a_ic|).  But on `cluster` and `shifted` the FAR pairs set uS_c, through
|W| dg D_c^2 with dsq >= (k + 2) eps (nrm_i + nrm_j) - the error the norm + GEMM distance is allowed - and the variant
reaches 2e-4 and 6e-4 units there.  It shows where exp(-sqrt5 d) removes the far pairs from S_c and from uS_c alike:
`pairs_case`, two clusters 1e-6 wide at -1 and +1 under lengthscales of 0.05, where the close pairs carry the sum
(1e4 to 1e5 units; the direct square stays below 0.1).  Those states are part of the device grid.
"""
import math
from types import SimpleNamespace

import numpy as np

import gp_reference as G
from wpca_reference import EPS, EXTENDED, f64, hp, hp_log, hp_sqrt

HOST = 8.0 * EPS
S5 = math.sqrt(5.0)
LOG2PI = 1.8378770664093453
FOLD_FLOOR = 2.0 ** -40
BS = 64
ARD_CHUNK = 8
QUANTITIES = ("loss", "g_noise", "g_mean", "g_rho")
SUMS = ("h0", "h1", "h2", "h3", "h4", "S")
THETA0 = (math.exp(-5.0), 0.0, 0.0)

# ---- thetas and states of the two test files ------------------------------------------------------------------------
SCALAR_THETAS = ((math.exp(-5.0), 0.0, 0.0), (1e-4, 0.3, -0.5), (0.05, -0.2, 0.8), (0.3, 0.5, 3.0), (0.05, 0.3, 20.5))
GRID_N = (257, 193, 129, 128, 65, 64, 63, 17, 3, 2)
GRID_N_K = (1, 5)
GRID_K = (128, 65, 64, 33, 12, 9, 8, 5, 4, 3, 1)
GRID_K_N = (129, 65)
N_BELOW_K = (20, 100)
GEN_SHAPES = ((129, 33), (65, 5))
GRID_PARTS = ("n-k1", "n-k5", "k-n129", "k-n65", "generators", "pairs")
# two tight, far-apart clusters under short lengthscales: the states on which an expanded square in S_c shows (below)
PAIRS_SHAPES = ((129, 33), (65, 5), (17, 3))
PAIRS_WIDTH, PAIRS_LS, PAIRS_S2, PAIRS_C = 1e-6, 0.05, 0.05, 0.3
# the CPU grid of the restatement (test_mll_reference_cpu.py, a)
CPU_N, CPU_K = (3, 64, 65, 129), (1, 5, 33, 128)
CPU_HYPERS = ((G.LENGTHSCALE, math.exp(-5.0)), (0.2, 1e-4), (3.0, 0.05))
CPU_MEAN_C = 0.3


def grid_part(part):
    """(gen, n, k) of one part of the device grid, large problems first."""
    if part.startswith("n-k"):
        k = int(part[3:])
        return [("lhs", n, k) for n in GRID_N]
    if part.startswith("k-n"):
        n = int(part[3:])
        return [("lhs", n, k) for k in GRID_K] + ([("lhs",) + N_BELOW_K] if n == GRID_K_N[-1] else [])
    if part == "pairs":
        return [("pairs", n, k) for n, k in PAIRS_SHAPES]
    return [(gen, n, k) for n, k in GEN_SHAPES for gen in G.GENERATORS]


def pairs_case(n, k):
    """Points alternating between two clusters at -1 and +1 in every input, each PAIRS_WIDTH wide.  Under a lengthscale of
    PAIRS_LS of the Normalize range exp(-sqrt5 d) removes the pairs across the clusters (d = 16 sqrt k) from S_c and from
    its unit; the pairs inside a cluster carry both, with |a_ic| ~ 8 and |D_c| ~ 1e-5: the state on which the direct square
    of S_c matters."""
    rng = np.random.default_rng([n, k, 4712])
    Z = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)[:, None] + PAIRS_WIDTH * rng.uniform(-0.5, 0.5, size=(n, k))
    y = rng.normal(size=n) * 200.0 + 900.0
    return SimpleNamespace(gen="pairs", n=n, k=k, hyper="default", Z=np.ascontiguousarray(Z), y=y, lengthscale=G.LENGTHSCALE,
                           noise=G.NOISE, kernel="matern", norm_bounds=None, id="pairs-n%d-k%d" % (n, k))


def make_case(gen, n, k):
    return pairs_case(n, k) if gen == "pairs" else G.make_case(gen, n, k)


def pairs_theta(form, k):
    rho = math.log(math.expm1(PAIRS_LS))
    return np.r_[PAIRS_S2, PAIRS_C, np.full(k if form == "ard" else 1, rho)]


def ard_thetas(n, k):
    """The start; seeded rho in [-1.5, 2] with c != 0; the noise at its bound; one rho_c = 15; one rho_c = 25 (softplus's
    linear branch) - the thetas of test_gpu_ard.py, restated - and one with a rho_c = 20.5."""
    rng = np.random.default_rng(1000 * n + k)
    rho = rng.uniform(-1.5, 2.0, size=k)
    c = int(rng.integers(k))
    big, lin, thr = rho.copy(), rho.copy(), rho.copy()
    big[c], lin[c], thr[(c + 1) % k] = 15.0, 25.0, 20.5
    return [np.r_[THETA0[0], THETA0[1], np.zeros(k)], np.r_[0.05, 0.3, rho], np.r_[1e-4, -0.2, rho],
            np.r_[0.05, 0.3, big], np.r_[0.02, -0.1, lin], np.r_[0.05, 0.3, thr]]


def thetas(form, n, k, gen="lhs"):
    if gen == "pairs":
        return [pairs_theta(form, k)]
    return [np.asarray(t, dtype=np.float64) for t in (SCALAR_THETAS if form == "scalar" else ard_thetas(n, k))]


def fit_state(seed, n, k):
    """A state with something to fit: Z ~ U(-2, 2)^k, y = sin(3 z0) + (z0^2 + z1^2) / 2 + 0.1 noise."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-2.0, 2.0, size=(n, k))
    y = np.sin(3.0 * Z[:, 0]) + 0.5 * (Z[:, :2] ** 2).sum(axis=1) + 0.1 * rng.standard_normal(n)
    return Z, y


def softplus64(rho):
    """The lengthscales as the library computes them: fp64, torch's threshold."""
    rho = np.asarray(rho, dtype=np.float64)
    return np.where(rho > 20.0, rho, np.log1p(np.exp(np.minimum(rho, 20.0))))


def data_bounds(Z):
    """Normalize's bounds of the data in fp64, as `k_zstats` and `gp_reference.restate` compute them."""
    zmin, zmax = Z.min(axis=0), Z.max(axis=0)
    rng = zmax - zmin
    return zmin - 0.1 * rng, zmax + 0.1 * rng


def fold(lo, hi, ls):
    """`k_zstats`' fold of the ARD lengthscales into the Normalize ranges, and whether its 2^-40 floor is active."""
    floor = np.maximum(np.abs(lo), hi - lo) * FOLD_FLOOR
    return lo + np.maximum((hi - lo) * ls, floor), bool(np.any((hi - lo) * ls <= floor))


def host_state(case, theta, ard, **wrong):
    """A state conditioned at theta on the host: `gp_reference.restate` at theta's lengthscale and noise (ARD: on the
    folded bounds at lengthscale 1), alpha recomputed for y_s - c."""
    theta = np.asarray(theta, dtype=np.float64)
    cs = SimpleNamespace(**case.__dict__)
    cs.noise, cs.kernel = float(theta[0]), "matern"
    if ard:
        lo, hi = data_bounds(case.Z)
        hi2, floored = fold(lo, hi, softplus64(theta[2:]))
        assert not floored, "the 2^-40 floor of k_zstats is active on this state"
        cs.norm_bounds, cs.lengthscale = np.vstack([lo, hi2]), 1.0
    else:
        cs.norm_bounds, cs.lengthscale = None, float(softplus64(theta[2]))
    res = G.restate(cs, **wrong)
    m1 = res.y_mean if theta[1] == 0.0 else res.y_mean + res.y_std * theta[1]
    ys = (case.y - m1) / res.y_std
    return {"L": res.L, "R": res.R, "alpha": res.R.T @ (res.R @ ys), "y_mean": m1, "y_std": res.y_std,
            "norm_bounds": res.norm_bounds}


# ---- arithmetic: long double, or mpmath --------------------------------------------------------------------------------
def _ld_arith():
    one = np.longdouble(1.0)
    return SimpleNamespace(conv=hp, exp=G.hp_exp, sqrt=hp_sqrt, log=hp_log, log1p=np.log1p if EXTENDED else None,
                           pi=4 * np.arctan(one), dps=None)


def mp_arith(dps):
    """The formulas on mpmath objects with `dps` digits (use inside `mpmath.workdps(dps)`)."""
    import mpmath
    fn = {name: np.frompyfunc(getattr(mpmath, name), 1, 1) for name in ("mpf", "exp", "sqrt", "log", "log1p")}

    def conv(a):
        return fn["mpf"](np.asarray(f64(a), dtype=object))

    return SimpleNamespace(conv=conv, exp=fn["exp"], sqrt=fn["sqrt"], log=fn["log"], log1p=fn["log1p"], pi=mpmath.pi,
                           dps=dps)


def _arith():
    return _ld_arith() if EXTENDED else mp_arith(30)                    # pragma: no cover - the second, not on x86


def _softplus(X, rho):
    """(l, dl / drho) per rho in the arithmetic X: torch's threshold, the derivative of what is evaluated."""
    ls, slope = [], []
    for r in np.atleast_1d(rho):
        x = X.conv(float(r))
        if float(r) > 20.0:
            ls.append(x)
            slope.append(X.conv(1.0))
        else:
            ls.append(X.log1p(X.exp(x)))
            slope.append(1 / (1 + X.exp(-x)))
    return ls, slope


def _assemble(X, n, h, S, theta, ls, slope):
    s2 = X.conv(float(theta[0]))
    lnz = X.log(s2)
    u = lnz + 4
    l2pi = X.log(2 * X.pi)
    loss = (h[1] / 2 + h[0] + n * l2pi / 2 + lnz + l2pi / 2 + u * u / 2) / n
    grad = [-((h[3] - h[4]) / 2 - (1 + u) / s2) / n, -h[2] / n]
    grad += [-(S[j] / 2 * slope[j] / ls[j]) / n for j in range(len(S))]
    return loss, grad


def sums(state, Z, y, theta, ard, arith=None):
    """h0 .. h4, S (m values), loss and grad (2 + m) of the formulas in the module docstring, with the arrays the
    units are made of.  `state` may hold extended-precision arrays (a state conditioned in long double)."""
    X = arith or _arith()
    c = X.conv
    Z = np.asarray(Z, dtype=np.float64)
    n, k = Z.shape
    if not EXTENDED and X.dps is None and n > G.MP_MAX_N:                # pragma: no cover
        return SimpleNamespace(skip="np.longdouble is a plain double here and n = %d is beyond the mpmath path" % n)
    theta = np.asarray(theta, dtype=np.float64)
    m = k if ard else 1
    assert theta.shape == (2 + m,)
    L, R, alpha = c(state["L"]), c(state["R"]), c(state["alpha"])
    m1, s = c(state["y_mean"]), c(state["y_std"])
    lo, hi = c(state["norm_bounds"][0]), c(state["norm_bounds"][1])
    ls, slope = _softplus(X, theta[2:])
    ys = (c(np.asarray(y, dtype=np.float64)) - m1) / s
    zn = (c(Z) - lo) / (hi - lo)
    a = zn if ard else zn / ls[0]
    sq, D = 0, []
    for col in range(k):
        d_c = a[:, col, None] - a[None, :, col]
        D.append(d_c)
        sq = sq + d_c * d_c
    s5 = X.sqrt(c(5.0))
    d = X.sqrt(sq)
    g = c(5.0) / c(3.0) * (1 + s5 * d) * X.exp(-s5 * d)
    w = g * sq
    Kinv = R.T @ R
    W = alpha[:, None] * alpha[None, :] - Kinv
    off = c(1.0 - np.eye(n))
    h = [X.log(np.diagonal(L)).sum(), (ys * alpha).sum(), alpha.sum(), (alpha * alpha).sum(), np.trace(Kinv)]
    Wg = W * g * off
    S = [(Wg * (D[col] * D[col])).sum() for col in range(k)] if ard else [(W * w * off).sum()]
    loss, grad = _assemble(X, n, h, S, theta, ls, slope)
    return SimpleNamespace(skip=None, n=n, k=k, m=m, ard=ard, theta=theta, h=h, S=S, loss=loss, grad=grad, ls=ls,
                           slope=slope, ys=ys, zn=zn, a=a, sq=sq, d=d, g=g, w=w, W=W, Kinv=Kinv, alpha=alpha, L=L, R=R,
                           m1=m1, s=s, y=np.asarray(y, dtype=np.float64))


def reference(state, Z, y, theta, ard):
    """`sums` in extended precision with the units `u_h` (5), `u_S` (m), `u_loss`, `u_grad` (2 + m) and the term
    scales `t_grad` (the sums of the absolute terms of each gradient component)."""
    r = sums(state, Z, y, theta, ard)
    if r.skip:
        return r
    n, k, m = r.n, r.k, r.m
    theta = r.theta
    s2, mc = float(theta[0]), float(theta[1])
    lsf, slf = f64(r.ls), f64(r.slope)
    # -- the distance
    zn, a = f64(r.zn), r.a
    A = f64(a - a.sum(axis=0) / n)                      # centred, as the kernels hold them: the norms enter dsq
    delta = np.full(k, (3.0 if ard else 5.0) * EPS)
    dsq, e = G.dsq_bound(A, zn, delta, 1.0 if ard else float(lsf[0]))
    SQ = f64(r.sq)
    Dd = np.sqrt(SQ)
    sq_lo = np.maximum(SQ - dsq, 0.0)
    off = 1.0 - np.eye(n)
    # -- W
    Wf, al, aR = np.abs(f64(r.W)), np.abs(f64(r.alpha)), np.abs(f64(r.R))
    aa = np.outer(al, al)
    dW = (n + 2) * EPS * (aR.T @ aR) + 2.0 * EPS * aa + EPS * Wf
    depth = (2 * n + 4) * EPS
    if ard:
        gf = np.abs(f64(r.g))
        dg = 25.0 / 6.0 * np.exp(-S5 * np.sqrt(sq_lo)) * dsq + EPS * gf * (5.0 + S5 * Dd)
        u_S, t_S = np.zeros(k), np.zeros(k)
        for col in range(k):
            Dc = np.abs(A[:, col, None] - A[None, :, col])
            D2 = Dc * Dc
            dD2 = 2.0 * Dc * (e[:, col, None] + e[None, :, col]) + 2.0 * (delta[col] + EPS) * D2
            t = gf * D2
            t_S[col] = (Wf * t * off).sum()
            u_S[col] = ((Wf * (dg * D2 + gf * dD2) + t * dW) * off).sum() + depth * t_S[col]
    else:
        def slope_w(sq):
            dd = np.sqrt(sq)
            return np.abs(5.0 / 3.0 * np.exp(-S5 * dd) * (1.0 + S5 * dd - 2.5 * sq))

        wf = np.abs(f64(r.w))
        dw = np.maximum(np.maximum(slope_w(sq_lo), slope_w(SQ)), slope_w(SQ + dsq)) * dsq + EPS * wf * (6.0 + S5 * Dd)
        t_S = np.array([(Wf * wf * off).sum()])
        u_S = np.array([((Wf * dw + wf * dW) * off).sum() + depth * t_S[0]])
    # -- h0 .. h4
    h = f64(np.array(r.h, dtype=object))
    ysf, yf = np.abs(f64(r.ys)), np.abs(r.y)
    sf, m1f = float(f64(r.s)), abs(float(f64(r.m1)))
    u_ys = EPS * ((yf + m1f) / sf + 3.0 * ysf + abs(mc))
    u_h = np.array([(n + 3) * EPS * np.abs(np.log(np.diag(f64(r.L)))).sum(),
                    (n + 2) * EPS * (ysf * al).sum() + (al * u_ys).sum(),
                    (n + 2) * EPS * al.sum(), (n + 2) * EPS * h[3], (2 * n + 4) * EPS * h[4]])
    # -- loss and gradient
    lnz = math.log(s2)
    u = lnz + 4.0
    Sf = f64(np.array(r.S, dtype=object))
    r.u_h, r.u_S, r.t_S = u_h, u_S, t_S
    r.u_loss = (u_h[0] + 0.5 * u_h[1]) / n + HOST * (abs(h[0]) + 0.5 * abs(h[1]) + 0.5 * n * LOG2PI + abs(lnz)
                                                   + 0.5 * LOG2PI + 0.5 * u * u + abs(u * lnz)) / n
    chain = slf / lsf / n
    r.u_grad = np.r_[(0.5 * (u_h[3] + u_h[4]) + HOST * (0.5 * (h[3] + h[4]) + (1.0 + abs(u) + abs(lnz)) / s2)) / n,
                     (u_h[2] + HOST * abs(h[2])) / n, (0.5 * u_S + 0.5 * HOST * np.abs(Sf)) * chain]
    r.t_grad = np.r_[(0.5 * (h[3] + h[4]) + (1.0 + abs(u)) / s2) / n, al.sum() / n, 0.5 * t_S * chain]
    return r


# ---- judging ------------------------------------------------------------------------------------------------------------
def _ratio(err, unit, n):
    """|err| / unit; NaN, or an error where the unit is 0, counts as infinite; up to n 2^-1022 counts as none."""
    err, unit = abs(float(err)), float(unit)
    if not math.isfinite(err) or not math.isfinite(unit):
        return float("inf")
    if err <= n * G.UNDERFLOW:
        return 0.0
    return err / unit if unit > 0.0 else float("inf")


def judge(ref, loss, grad):
    """Ratios of a loss and gradient to the units of `ref`: `loss`, `g_noise`, `g_mean`, `g_rho` (ARD: the worst
    component, `rho_index`)."""
    grad = np.asarray(grad, dtype=np.float64)
    assert grad.shape == (2 + ref.m,)
    X = _arith()
    rat = [_ratio(X.conv(float(grad[j])) - ref.grad[j], ref.u_grad[j], ref.n) for j in range(2 + ref.m)]
    worst = int(np.argmax(rat[2:]))
    return SimpleNamespace(loss=_ratio(X.conv(float(loss)) - ref.loss, ref.u_loss, ref.n), g_noise=rat[0], g_mean=rat[1],
                           g_rho=rat[2 + worst], rho_index=worst, rho_all=rat[2:])


def judge_sums(ref, h):
    """Ratios of the 5 + m sums to `u_h` and `u_S`: h0 .. h4 and `S` (ARD: the worst S_c, `S_index`)."""
    X = _arith()
    h = np.asarray(h, dtype=np.float64)
    assert h.shape == (5 + ref.m,)
    out = SimpleNamespace(**{"h%d" % j: _ratio(X.conv(float(h[j])) - ref.h[j], ref.u_h[j], ref.n) for j in range(5)})
    rat = [_ratio(X.conv(float(h[5 + j])) - ref.S[j], ref.u_S[j], ref.n) for j in range(ref.m)]
    out.S_index = int(np.argmax(rat))
    out.S, out.S_all = rat[out.S_index], rat
    return out


class Worst:
    """Worst ratio per row label and quantity, for the tables the tests print."""

    def __init__(self, quantities=QUANTITIES):
        self.q, self.w = quantities, {}

    def add(self, row, j, case_id):
        for q in self.q:
            v = getattr(j, q)
            if (row, q) not in self.w or not v <= self.w[(row, q)][0]:
                self.w[(row, q)] = (float(v), case_id)

    def failures(self, limit):
        return [(cid, q, v) for (_, q), (v, cid) in self.w.items() if not v <= limit]

    def table(self, title):
        rows = sorted({row for row, _ in self.w})
        lines = [title, "%-12s" % "" + "".join("%11s" % q for q in self.q)]
        for row in rows:
            lines.append("%-12s" % row + "".join("%11.3g" % self.w[(row, q)][0] for q in self.q))
        for q in self.q:
            v, cid = max((self.w[(row, q)] for row in rows), key=lambda t: t[0] if t[0] == t[0] else float("inf"))
            lines.append("  worst %-8s %10.3g  %s" % (q, v, cid))
        return "\n".join(lines)


def case_id(case, form, theta):
    return "%s-%s-s2=%.3g-c=%.3g-rho=%s" % (case.id, form, theta[0], theta[1],
                                           "%.3g" % theta[2] if len(theta) == 3 else "[%.3g..%.3g]" % (theta[2:].min(), theta[2:].max()))


# ---- the documented algorithm in plain fp64 -----------------------------------------------------------------------------
def restate_sums(state, Z, y, theta, ard, trace_padded=False, tile10_once=False, skip_first_row=False,
                 coef53=5.0 / 3.0, expanded_square=False, drop_second_chunk=False, shift_slots=False):
    """The 5 + m sums as the kernels form them, in numpy fp64: a centred with the mean of the raw points, the norm +
    GEMM distance with the 1e-30 floor under the root, K^-1 = R^T R tile by tile over the rows p >= 64 I, off-diagonal
    tiles counted twice.  One wrong variant per keyword: the trace over the padded NP rows (identity padding);
    tile (1, 0) counted once; the first row of R's block I left out of K^-1; 5/3 as a float; ARD: the square
    expanded as a_i^2 + a_j^2 - 2 a_i a_j, the inputs c >= 8 dropped (the second chunk of eight), S_c in slot c + 1."""
    Z, y = np.asarray(Z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    n, k = Z.shape
    m = k if ard else 1
    L, R, alpha = state["L"], state["R"], state["alpha"]
    lo, hi = state["norm_bounds"]
    ys = (y - state["y_mean"]) / state["y_std"]
    inv_ls = 1.0 if ard else 1.0 / float(softplus64(theta[2]))
    zn = (Z - lo) / (hi - lo)
    A = (zn - (Z.sum(axis=0) / n - lo) / (hi - lo)) * inv_ls
    nrm = (A * A).sum(axis=1)
    c53 = float(coef53)
    S, tr = np.zeros(m), 0.0
    nb = -(-n // BS)
    for bi in range(nb):
        ri = slice(BS * bi, min(BS * bi + BS, n))
        p0 = BS * bi + (1 if skip_first_row else 0)
        for bj in range(bi + 1):
            cj = slice(BS * bj, min(BS * bj + BS, n))
            kinv = R[p0:n, ri].T @ R[p0:n, cj]
            sq = (nrm[ri, None] + nrm[None, cj]) - 2.0 * (A[ri] @ A[cj].T)
            sq = np.maximum(sq, 0.0)
            dist = np.sqrt(np.maximum(sq, 1e-30))
            Wt = alpha[ri, None] * alpha[None, cj] - kinv
            mask = np.ones_like(Wt)
            if bi == bj:
                np.fill_diagonal(mask, 0.0)
                tr += np.diag(kinv).sum()
            f = 1.0 if bi == bj or (tile10_once and (bi, bj) == (1, 0)) else 2.0
            if ard:
                g = Wt * (c53 * (1.0 + S5 * dist) * np.exp(-S5 * dist)) * mask
                for col in range(min(k, ARD_CHUNK) if drop_second_chunk else k):
                    ai, bc = A[ri, col, None], A[None, cj, col]
                    d2 = (ai * ai + bc * bc) - 2.0 * (ai * bc) if expanded_square else (ai - bc) * (ai - bc)
                    S[col] += f * (g * d2).sum()
            else:
                S[0] += f * (Wt * (c53 * (dist * dist) * (1.0 + S5 * dist) * np.exp(-S5 * dist)) * mask).sum()
    if trace_padded:
        tr += nb * BS - n
    if shift_slots:
        S = np.r_[0.0, S[:-1]]
    return np.r_[np.log(np.diag(L)).sum(), ys @ alpha, alpha.sum(), alpha @ alpha, tr, S]


def restate_assemble(h, n, theta, ard, sigmoid_above_threshold=False):
    """`mll_assemble` in numpy fp64.  `sigmoid_above_threshold`: the scalar form's slope before it was corrected -
    the sigmoid where the loss takes l = rho."""
    theta = np.asarray(theta, dtype=np.float64)
    s2 = theta[0]
    lnz = math.log(s2)
    u = lnz + 4.0
    log_n = -0.5 * h[1] - h[0] - 0.5 * n * LOG2PI
    log_prior = -lnz - 0.5 * LOG2PI - 0.5 * u * u
    loss = -(log_n + log_prior) / n
    grad = [-((0.5 * (h[3] - h[4])) + (-1.0 - u) / s2) / n, -h[2] / n]
    for j, rho in enumerate(theta[2:]):
        ls = float(softplus64(rho))
        sig = 1.0 if rho > 20.0 and not sigmoid_above_threshold else 1.0 / (1.0 + math.exp(-rho))
        grad.append(-(0.5 * h[5 + j] * sig / ls) / n)
    return loss, np.array(grad)


# ---- the loss with no state at all ---------------------------------------------------------------------------------------
def scratch_bounds(Z):
    """Normalize's bounds of the data in extended precision."""
    zmin, zmax = hp(Z.min(axis=0)), hp(Z.max(axis=0))
    return zmin - hp(0.1) * (zmax - zmin), zmax + hp(0.1) * (zmax - zmin)


def _scratch(Z, y, theta, ard):
    """Normalize, Gram, `hp_cholesky`, root inverse, alpha and the loss at theta, all in extended precision; theta may
    hold extended-precision values (the difference quotients move it by less than an fp64 can say)."""
    X = _ld_arith()
    n, k = Z.shape
    th = [t if isinstance(t, np.longdouble) else hp(float(t)) for t in theta]
    s2, mc = th[0], th[1]
    ls = [r if float(r) > 20.0 else np.log1p(np.exp(r)) for r in th[2:]]
    lo, hi = scratch_bounds(Z)
    zn = (hp(Z) - lo) / (hi - lo)
    a = zn / (np.array(ls, dtype=np.longdouble) if ard else ls[0])
    sq = G.hp_zeros((n, n))
    for col in range(k):
        d_c = a[:, col, None] - a[None, :, col]
        sq = sq + d_c * d_c
    s5, d = hp_sqrt(hp(5.0)), hp_sqrt(sq)
    K = (1 + s5 * d + hp(5.0) / hp(3.0) * sq) * np.exp(-s5 * d) + s2 * hp(np.eye(n))
    yh = hp(y)
    ym = yh.sum() / n
    sd = hp_sqrt(((yh - ym) ** 2).sum() / (n - 1))
    ys = (yh - ym) / sd - mc
    L = G.hp_cholesky(K)
    R = G.hp_lower_inverse(L)
    alpha = R.T @ (R @ ys)
    lnz = np.log(s2)
    u = lnz + 4
    l2pi = np.log(2 * X.pi)
    loss = ((ys * alpha).sum() / 2 + np.log(np.diagonal(L)).sum() + n * l2pi / 2 + lnz + l2pi / 2 + u * u / 2) / n
    return loss, L, R, alpha, ym, sd, lo, hi, ls


def loss_from_scratch(Z, y, theta, ard):
    return _scratch(np.asarray(Z, dtype=np.float64), np.asarray(y, dtype=np.float64), theta, ard)[0]


def scratch_state(Z, y, theta, ard):
    """The state of `_scratch` in extended precision, in the layout `sums` reads (ARD: the lengthscales folded into
    the bounds, y_mean = m + s c)."""
    _, L, R, alpha, ym, sd, lo, hi, ls = _scratch(np.asarray(Z, dtype=np.float64), np.asarray(y, dtype=np.float64), theta, ard)
    if ard:
        hi = lo + (hi - lo) * np.array(ls, dtype=np.longdouble)
    return {"L": L, "R": R, "alpha": alpha, "y_mean": ym + sd * hp(float(theta[1])), "y_std": sd, "norm_bounds": (lo, hi)}


def richardson(f, x, j, h):
    """d f / d x_j by central differences at h and h / 2, extrapolated: the error is O(h^4)."""
    def central(step):
        xp, xm = list(x), list(x)
        xp[j], xm[j] = x[j] + step, x[j] - step
        return (f(xp) - f(xm)) / (2 * step)
    return (4 * central(h / 2) - central(h)) / 3
