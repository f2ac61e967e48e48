"""Extended-precision reference of log-EI, PI, UCB and the posterior query on a conditioned GP and the error units
their results are judged in.

No tests here: `test_acq_reference_cpu.py` and `test_ucb_posterior_reference_cpu.py` prove the reference and its units
on a plain numpy restatement, `test_gpu_acq_edges.py` and `test_gpu_ucb_edges.py` judge the HIP kernels that evaluate
the acquisition (`k_acq_fast`, `k_acq_fused`, `k_acq_group`, `k_acq_combine`, the GEMM scoring of kernels_acq.hip and
`lb_eval` of kernels_lbfgsb.hip, all on the scalar maths of acq_math.h) by them, `test_gpu_posterior_edges.py` the
posterior query (`k_post_combine`, `k_post_cov` of kernels_post.hip behind the scoring's first two launches).

The reference starts from a CONDITIONED state {R, alpha, y_mean, y_std, norm_bounds}, fp64 arrays taken as exact (the
conditioning has its own judge: gp_reference.py), so nothing of the conditioning's kappa-type factors enters.  For a
query x, training points Z (n x k), lengthscale l:
  xn = (x - lo) / (hi - lo),  zn likewise,  d_jc = xn_c - zn_jc,  sq_j = sum_c d_jc^2 / l^2      (the direct form)
  ks_j = (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r), r = sqrt(sq_j)  (Matern-5/2)   or   exp(-sq_j / 2)  (RBF)
  cf_j: dks_j/dxn = cf_j d_j, cf_j = -5/3 (1 + sqrt5 r) exp(-sqrt5 r) / l^2   or   -ks_j / l^2
  v = R ks,  vv = |v|^2,  mus = alpha . ks,  w = R^T v
  A_c = sum_j alpha_j cf_j d_jc / (hi_c - lo_c),   B_c = sum_j w_j cf_j d_jc / (hi_c - lo_c)
in `np.longdouble` (`linear()`), then per query in `mpmath` (80 digits), from the definitions and not from botorch's
rearrangement (`scalars()`):
  mu = y_mean + y_std mus,  var = (1 - vv) y_std^2 floored at 1e-10 (the query is then CLAMPED),  sigma = sqrt(var)
  u = +-(mu - best_f) / sigma          (+ where maximising)
  log-EI = log(phi(u) + u Phi(u)) + log sigma,    PI = Phi(u)
  g_c = c_mu A_c + c_sg B_c,   c_mu = (dval/du)(+-y_std / sigma),
  c_sg = ([log-EI] 1 / sigma - (dval/du) u / sigma)(-y_std^2 / sigma), 0 where clamped.
For u <= -1e6 the kernels take botorch's asymptote; it is O(1 / u^2) absolute off a value of order u^2 / 2, far inside
the unit there, so the exact value stays the reference.

Error units: first-order bounds of what ANY fp64 implementation of this chain commits (eps = 2^-52), computed from
reference quantities only - never from a run of the code under test.
  dd_jc = 2 eps (|xn_c| + |zn_jc|) + eps |d_jc|
  dsq_j = (2 sum_c |d_jc| dd_jc + (k + 2) eps sum_c d_jc^2) / l^2 + 3 eps sq_j
  dks_j = |dks/dsq| dsq_j + eps |ks_j| (4 + arg),  arg = sqrt5 r  or  sq / 2  (as u_K of gp_reference)
  dcf_j = |dcf/dsq| dsq_j + eps |cf_j| (4 + arg),  |dcf/dsq| = 25/6 exp(-sqrt5 r) / l^2  or  |ks| / 2 / l^2
  dmus = sum |alpha_j| dks_j + (n + 2) eps sum |alpha_j ks_j|
  dv = |R| dks + (n + 2) eps |R||ks|,   dvv = 2 sum |v_i| dv_i + (n + 2) eps vv
  dw = |R^T| dv + (n + 2) eps |R^T||v|
  dA_c, dB_c: the product rule over alpha_j (w_j +- dw_j), cf_j +- dcf_j, d_jc +- dd_jc, + (n + 4) eps sum of |terms|
  dmu = y_std dmus + 2 eps (|y_mean| + |y_std mus|),   dvar = y_std^2 (dvv + eps (1 + 3 |1 - vv|))
  dsigma = dvar / (2 sigma) + eps sigma  (0 where clamped)
  du = (dmu + eps |mu - best_f|) / sigma + |u| dsigma / sigma + 2 eps |u|
log-EI helper h(u) = log(phi + u Phi), by the branch of acq_math.h's `log_ei_helper` (`helper_units`):
  u > -1:          dei = eps (phi (2 + u^2) + 3 |u| Phi + ei),  u_h = dei / ei + eps |h|,  u_dh = h' (3 eps + dei / ei)
  -1e6 < u <= -1:  with E = erfcx(-u / sqrt2) |u| sqrt(pi / 2), 1 - E and dw = u + sqrt(2 / pi) / erfcx + 1 / u EXACT,
                   u_h = 2 eps (u^2 / 2 + 1) + 4 eps E / (1 - E) + eps |log(1 - E)|
                   u_dh = eps |u| + 5 eps |u| E / (1 - E) + |dw| E / (1 - E) (4 eps + (4 eps E + eps) / (1 - E) + 3 eps)
                   (dw cancels from |u| down to 2 / |u|^3, E / (1 - E) ~ u^2: u_dh grows as 5 eps |u|^3 - that is
                   botorch's formulation, which the kernels follow, and not a bug)
  u <= -1e6:       u_h = 2 eps (u^2 / 2 + 2 log |u| + 2),  u_dh = 2 eps |u|
a query whose u lies within du of a seam takes the larger unit of the two branches.
  value: log-EI |h'| du + u_h + dsigma / sigma + eps (|log sigma| + |value|);  PI phi (du + 2 eps |u|) + 4 eps Phi
  d(dval/du) = |d2val/du2| du + u_dh,  h'' = phi / ei - h'^2;   PI: |u| phi du + eps phi (3 + u^2)
  dc_mu = (y_std / sigma)(d(dval/du) + |dval/du| (dsigma / sigma + 3 eps))
  T = [log-EI] 1 / sigma - (dval/du) u / sigma,  c_sg = -T y_std^2 / sigma:
  dT = [log-EI] (dsigma / sigma^2 + eps / sigma) + (d(dval/du) |u| + |dval/du| du + |dval/du u| (dsigma / sigma + 3 eps)) / sigma + eps |T|
  dc_sg = (y_std^2 / sigma)(dT + |T| (dsigma / sigma + 3 eps))
  dg_c = |c_mu| dA_c + |A_c| dc_mu + |c_sg| dB_c + |B_c| dc_sg + 2 eps (|c_mu A_c| + |c_sg B_c|)
Underflow: as in gp_reference, an error up to 2^-1022 per element counts as none (PI and its gradient are 0 in fp64
below u ~ -38).  `judge()` returns the worst ratio of values and of gradients; a NaN, or an error where the unit is
0, is infinite.

UCB (`scalars_ucb`; acq_math.h's `acq == 2` branch, kappa >= 0 in the best_f slot) and the posterior query
(`posterior`) are linear in the quantities of `linear()`, so they stay in long double and need no mpmath:
  value = +-mu + kappa sigma,   c_mu = +-y_std,   c_sg = -kappa y_std^2 / sigma (0 where clamped),   g = c_mu A + c_sg B
  u_value = dmu + kappa dsigma + eps (|kappa sigma| + |value|)       (the product and the sum, fused or not)
  dc_mu = eps |c_mu|,   dc_sg = |c_sg| (dsigma / sigma + 3 eps)  (the square, the division, the product),   dg as above
at a clamped variance sigma is sqrt(1e-10) whatever vv is: dsigma = 0, c_sg = dc_sg = 0, and the kappa term moves no
gradient bit.
  mean = y_mean + y_std mus                                     unit dmu
  raw variance = ((1 - vv) [+ s2]) y_std^2                      unit dvar [+ eps y_std^2 (s2 + |1 - vv + s2|): one more sum]
  variance = the raw one, or exactly 1e-10 (unit 0) where the raw one is below the floor - no raw variance, latent or
             noisy, may lie within VAR_MARGIN units of it (`check_posterior_conditions`), so the side is never rounding's
  cov_ab = y_std^2 (kq_ab [+ s2 delta_ab] - v_a . v_b), not floored; its diagonal is the raw variance with that unit
  kq_ab = k(xn_a, xn_b) in the direct form; dkq_ab is dks with both points queries:
          dd_c = 2 eps (|xn_ac| + |xn_bc|) + eps |d_c|,  dsq, dkq as dsq_j, dks_j above
  d(v_a . v_b) = sum_i (|v_ai| dv_bi + |v_bi| dv_ai) + (n + 2) eps sum_i |v_ai v_bi|
          (each factor off by its dv, and an n-term sum in any order; zero padding of v adds exact zeros)
  u_cov_ab = y_std^2 (dkq_ab + d(v_a . v_b) + eps |kq_ab - v_a . v_b|) + 3 eps |cov_ab|
          (the subtraction; y_std^2 and the product)
The unit of an off-diagonal entry does not shrink with the entry: where kq - v_a . v_b cancels (a duplicated query,
queries 1e-9 apart, a query on a training point) the error is held absolutely, at eps times the terms that cancel.
There the slope of k in sq is largest (5/6, 1/2) and sq itself ~ 1e-18, so a distance formed as |a|^2 + |b|^2 - 2 a.b
shows: it is off by roundings of |xn|^2 / l^2, not of sq.  That is a few eps at k = 1 - inside the unit, the norm form is
then as good as the direct one - and 28 units per rounding at k = 128.

The module also holds the states, queries and scalars of the test files (`make_state`, `cases`, `cases_ucb`), plain
fp64 numpy restatements of the chains written as the kernels are (`restate`, `restate_posterior`; keyword switches
turn on one wrong variant each), the conditions the device tests rely on (`check_conditions`,
`check_ucb_conditions`, `check_posterior_conditions`) and the cache of references on a device's own state that the
device test files share (`cached_linear`, `cached_scalars`, `cached_posterior`).

STATES ends with four states of the stress region (d = 100 runs: n = 300 .. 1050, k ~ 85; STRESS_STATES), each with
the code forms it is the first to reach and the arithmetic that puts them there: `k_acq_fused<32>` with k > 32,
`k_acq_group<2>` at k > 40 and with more than 64 KB of LDS, `k_acq_group<5>` with five live columns, the group context
beyond `acq_group_possible`, the second iteration of `grad_partial_sum`'s unrolled loop, `k_acq_combine` and
`k_post_combine` over more than 18 records, more than three `k_score_ks` blocks, more than nine row blocks of
`k_score_gemm` and panels of `k_post_cov`.  `test_gpu_optimize_edges.py` judges the optimiser's end points at k > 40
with the same reference.
"""
import hashlib
import math
from types import SimpleNamespace

import mpmath
import numpy as np

from gp_reference import _ratio, hp_exp
from wpca_reference import EPS, f64, hp, hp_sqrt

LOG_EI, PI, UCB = 0, 1, 2
LENGTHSCALE, NOISE = 0.6931471805599453, 0.006737946999085467      # the defaults of gp_condition
FLOOR = 1e-10                        # gpytorch's min_variance
Q = 130                              # queries per state
PREFIXES = (5, 6, 32, 40, 130)       # what the evaluation paths take of them
VAR_MARGIN = 32.0                    # no variance within this many dvar of the floor
SEAM_QUERY = 4                       # the query whose u the seam incumbents are computed for (its duplicate: 3)
FIXED_QUERIES = (0, 1, 2, 3, SEAM_QUERY)      # placed by hand in make_state, never redrawn
NEAR_PAIRS = ((6, 7), (SEAM_QUERY, 129))      # (a, b): query b is query a + 1e-9, in one covariance tile and across two
KAPPAS = (0.0, 0.5, math.sqrt(2.0), 1e3)      # UCB: the mean alone, two usual values, one where sigma carries everything
POST_PREFIXES = (1, 15, 16, 17, 63, 64, 65, 130)      # what the posterior queries take of the Q queries
MP = mpmath.mp.clone()
MP.dps = 80
_S5 = math.sqrt(5.0)

# state -> (n, k, scale of y, kernel, options): the smallest shapes that reach each code form.  A .. E are the states
# of test_gpu_ucb.py, with the same seeds.
STATES = {
    "A": (9, 1, 1.0, "matern52", {}),           # k_acq_fast, NP = 64, one component
    "B": (70, 6, 1.0, "matern52", {}),          # k_acq_fast, NP = 128, 16-row slabs
    "B-rbf": (70, 6, 1.0, "rbf", {}),
    "C": (449, 10, 1.0, "matern52", {}),        # k_acq_fast, NP = 512 (NB = 8), 32-row slabs; lb_eval with 2 row parts
    "D": (50, 41, 1.0, "matern52", {}),         # k_acq_fused (k > 40); host-paced paths only
    "E": (30, 3, 1e-7, "matern52", {}),         # every query's variance under the 1e-10 floor
    "n64": (64, 1, 1.0, "matern52", {}),        # NB = 1, an exact block
    "n65": (65, 3, 1.0, "matern52", {}),        # NB = 2 .. 7: every live k_acq_fast<SLAB, NB>, k cycling 1, 3, 8, 9, 40
    "n129": (129, 8, 1.0, "matern52", {}),
    "n193": (193, 9, 1.0, "matern52", {}),
    "n257": (257, 40, 1.0, "matern52", {}),
    "n321": (321, 1, 1.0, "matern52", {}),
    "n385": (385, 3, 1.0, "matern52", {}),
    "n513": (513, 6, 1.0, "matern52", {}),      # NP = 576 > 512: the generic kernel with 32-row slabs
    "k128": (100, 128, 1.0, "matern52", {}),    # k = PCABO_MAXD: the group kernel's widened LDS region
    "user": (100, 5, 1.0, "rbf", {"user_bounds": True, "lengthscale": 0.4, "noise": 1e-3}),
    "mixed": (30, 3, 1.2e-6, "matern52", {}),   # like E; clamped and free variances among the first 32 queries
    "T": (64, 3, 1.0, "matern52", {"tail_inputs": True}),     # Z and y of test_log_ei_tail_branches
    # The stress region (d = 100 runs: n = 300 .. 1050, k ~ 85).  NP = 64 ceil(n / 64); S = NP / 32 slabs of 32 rows;
    # a group of q queries passes q k coordinates, as kernel arguments up to PCABO_QA_MAX = 416 and through a pointer
    # beyond; k_acq_group<CPT> holds CPT = ceil(NP / 256) columns per thread and, by launch_acq_group's formula, needs
    # 65 568 bytes of dynamic LDS at (NP, k) = (512, 83) and 65 488 at k = 82: 83 is the smallest k past 64 KB there.
    # The two high-k states take a longer lengthscale than ln 2: at ln 2 a query in 65 normalised dimensions sees no
    # training point (median |v|^2 <= 2e-3), every gradient part through R is rounding-sized and a wrong R-part would
    # sit inside the unit; test_acq_reference_cpu.py holds their median |v|^2 to >= 0.01.
    #
    # n385k65, NP = 448 = ACQ_SLAB32_NP: k_acq_fused<32> with k > 32 - three trips of its gradient contraction
    # (c0 = 0, 32, 64 < 65), the second trip of acq_tail's and acq_finish_query's `c = l; c < k; c += 64` (c = 64)
    # and the c != l side of acq_tail's bounds selection; k_acq_group<2> (CPT = ceil(448 / 256)) at k > 40; k_post_cov's
    # second c0 += 64 trip over 7 panels of V; q k = 5 * 65 = 325 and 6 * 65 = 390 as kernel arguments, 32 * 65 = 2080
    # through the pointer; optimize_acqf on the host-paced paths at k > 40 (test_gpu_optimize_edges.py).
    "n385k65": (385, 65, 1.0, "matern52", {"lengthscale": 2.0}),
    # n449k83, NP = 512: k_acq_group<2> with 65 568 bytes of dynamic LDS, the smallest k past the 64 KB default;
    # q k = 5 * 83 = 415 of PCABO_QA_MAX = 416 as kernel arguments, 6 * 83 = 498 through the pointer; S = 16.
    "n449k83": (449, 83, 1.0, "matern52", {"lengthscale": 2.5}),
    # n1025, NP = 1088: k_acq_group<5> with all five columns per thread live (ceil(1088 / 256) = 5; n513 uses three);
    # S = 34 slabs, so k_acq_combine over S > 18 records; 17 row blocks of k_score_gemm (> 9), whose 17 records per
    # query k_post_combine adds; ceil(1088 / 256) = 5 blocks of k_score_ks (> 3); k_post_cov over 17 panels of V (> 9).
    "n1025": (1025, 5, 1.0, "matern52", {}),
    # n1473, NP = 1536 > 1280: beyond acq_group_possible, what a PCABO_OPT_GROUP_ACQ context does instead; S = 48 >= 46,
    # so grad_partial_sum's eight-at-a-time loop (`sl + 21 < S; sl += 24`) runs its second iteration; 6 blocks of
    # k_score_ks, 24 row blocks of k_score_gemm and so k_post_combine over 24 > 18 records, k_post_cov over 24 panels.
    "n1473": (1473, 2, 1.0, "matern52", {}),
}
SMALL_STATES = [s for s in STATES if STATES[s][0] <= 130]
STRESS_STATES = ["n385k65", "n449k83", "n1025", "n1473"]
HIGH_K_STATES = ["n385k65", "n449k83"]                   # the ones that carry their own lengthscale
# + two 256-column blocks of k_score_ks, and NP = 576; + the stress states: up to six blocks, 24 row blocks and panels
POSTERIOR_STATES = SMALL_STATES + ["n257", "n513"] + STRESS_STATES


# ---- states and queries ------------------------------------------------------------------------------------------
def search_box(Z):
    """The acquisition's search box of the points Z (include/pcabo.h, `pcabo_acq_bounds`), 2 x k."""
    zmin, zmax = Z.min(axis=0), Z.max(axis=0)
    b = np.vstack([zmin - 0.5 * (zmax - zmin), zmax + 0.5 * (zmax - zmin)])
    narrow = b[1] - b[0] < 0.1
    mid = (b[0] + b[1]) / 2
    b[0], b[1] = np.where(narrow, mid - 0.05, b[0]), np.where(narrow, mid + 0.05, b[1])
    return b


def make_state(name):
    """Seeded inputs of a state: the training points and values of test_gpu_ucb.py's recipe and Q queries, uniform in
    the search box widened by 20 %, with - inside every prefix the paths take - two training points (sq = 0 exactly),
    a training point + 1e-9 and a duplicated query; behind them the followers of NEAR_PAIRS, 1e-9 off their leaders."""
    n, k, yscale, kernel, opt = STATES[name]
    if opt.get("tail_inputs"):
        rng = np.random.default_rng(3)
        Z, y = rng.uniform(-1, 1, size=(n, k)), rng.normal(size=n)
    else:
        rng = np.random.default_rng(1000 + 10 * n + k)
        Z = rng.normal(size=(n, k))
        y = (rng.normal(size=n) * 30.0 + 200.0) * yscale
    st = SimpleNamespace(name=name, n=n, k=k, Z=np.ascontiguousarray(Z), y=y, kernel=kernel, norm_bounds=None,
                         lengthscale=opt.get("lengthscale", LENGTHSCALE), noise=opt.get("noise", NOISE))
    if opt.get("user_bounds"):
        st.norm_bounds = np.vstack([Z.min(axis=0) - 1.0, Z.max(axis=0) + 2.0])
    box = search_box(Z)
    wide = np.vstack([box[0] - 0.1 * (box[1] - box[0]), box[1] + 0.1 * (box[1] - box[0])])
    st.wide = wide
    st.qrng = np.random.default_rng(5000 + 10 * n + k)
    X = st.qrng.uniform(wide[0], wide[1], size=(Q, k))
    X[0], X[1] = Z[0], Z[1]
    X[2] = Z[2 % n] + 1e-9
    X[3] = X[4]
    for a, b in NEAR_PAIRS:
        X[b] = X[a] + 1e-9
    st.X = X
    st.redrawn = []
    return st


def restated_state(st):
    """The conditioned state of `st` from gp_reference's fp64 restatement (numpy's Cholesky): what the CPU proof uses
    where the device test reads the device's own state."""
    import gp_reference as G
    case = SimpleNamespace(Z=st.Z, y=st.y, lengthscale=st.lengthscale, noise=st.noise, norm_bounds=st.norm_bounds,
                           kernel="rbf" if st.kernel == "rbf" else "matern")
    r = G.restate(case)
    return {"R": r.R, "alpha": r.alpha, "y_mean": r.y_mean, "y_std": r.y_std, "norm_bounds": r.norm_bounds}


_PREPARED = {}


def prepared(name):
    """(state inputs, restated conditioned state, linear reference on it), once per process.  Queries whose variance
    - latent, or with the observation noise - lies within VAR_MARGIN dvar of the floor are REDRAWN here (never
    skipped), deterministically, so that all test files see the same queries; a follower of NEAR_PAIRS goes with its
    leader."""
    if name not in _PREPARED:
        st = make_state(name)
        gs = restated_state(st)
        lin = linear(st, gs, st.X)
        kept = set(FIXED_QUERIES) | {b for _, b in NEAR_PAIRS}
        for _ in range(20):
            near = [i for i in np.flatnonzero(near_floor(lin) | near_floor(lin, st.noise)) if i not in kept]
            if not near:
                break
            for i in near:
                st.X[i] = st.qrng.uniform(st.wide[0], st.wide[1])
                st.redrawn.append(int(i))
            for a, b in NEAR_PAIRS:
                st.X[b] = st.X[a] + 1e-9
            lin = linear(st, gs, st.X)
        _PREPARED[name] = (st, gs, lin)
    return _PREPARED[name]


# ---- the reference: linear algebra in long double ----------------------------------------------------------------
def _cov(sq, kernel, ls):
    """ks, cf, |dks/dsq|, |dcf/dsq|, arg of a scaled squared distance (any float type)."""
    il2 = 1 / (hp(ls) * hp(ls))
    if kernel == "rbf":
        ks = hp_exp(-sq / 2)
        return ks, -ks * il2, ks / 2, ks / 2 * il2, sq / 2
    r, s5 = hp_sqrt(sq), hp_sqrt(hp(5.0))
    e = hp_exp(-s5 * r)
    ks = (1 + s5 * r + hp(5.0) / hp(3.0) * sq) * e
    cf = -(hp(5.0) / hp(3.0)) * (1 + s5 * r) * e * il2
    return ks, cf, hp(5.0) / hp(6.0) * (1 + s5 * r) * e, hp(25.0) / hp(6.0) * e * il2, s5 * r


def linear(st, gs, X):
    """Everything of the chain that is linear algebra, for the queries X (q x k) on the conditioned state `gs`, in
    long double, with its units in fp64."""
    X = np.asarray(X, dtype=np.float64)
    q, k, n, ls = X.shape[0], st.k, st.n, float(st.lengthscale)
    R, alpha = hp(np.tril(gs["R"])), hp(gs["alpha"])
    lo, hi = hp(gs["norm_bounds"][0]), hp(gs["norm_bounds"][1])
    span = hi - lo
    xn, zn = (hp(X) - lo) / span, (hp(st.Z) - lo) / span
    d = xn[:, None, :] - zn[None, :, :]                                         # q x n x k
    ssq = (d * d).sum(axis=2)
    sq = ssq / (hp(ls) * hp(ls))
    ks, cf, dks_dsq, dcf_dsq, arg = _cov(sq, st.kernel, ls)
    v = ks @ R.T                                                                # v_i = sum_j R_ij ks_j
    vv = (v * v).sum(axis=1)
    mus = ks @ alpha
    w = v @ R                                                                   # w_j = sum_i R_ij v_i
    A = ((alpha[None, :] * cf)[:, :, None] * d).sum(axis=1) / span
    B = ((w * cf)[:, :, None] * d).sum(axis=1) / span
    # units, fp64
    aR, aal = np.abs(f64(R)), np.abs(f64(alpha))
    D, CF, KS, W, V = np.abs(f64(d)), np.abs(f64(cf)), np.abs(f64(ks)), np.abs(f64(w)), np.abs(f64(v))
    dd = 2.0 * EPS * (np.abs(f64(xn))[:, None, :] + np.abs(f64(zn))[None, :, :]) + EPS * D
    dsq = (2.0 * (D * dd).sum(axis=2) + (k + 2) * EPS * f64(ssq)) / (ls * ls) + 3.0 * EPS * f64(sq)
    dks = f64(dks_dsq) * dsq + EPS * KS * (4.0 + f64(arg))
    dcf = f64(dcf_dsq) * dsq + EPS * CF * (4.0 + f64(arg))
    dmus = dks @ aal + (n + 2) * EPS * (KS @ aal)
    dv = dks @ aR.T + (n + 2) * EPS * (KS @ aR.T)
    dvv = 2.0 * (V * dv).sum(axis=1) + (n + 2) * EPS * f64(vv)
    dw = dv @ aR + (n + 2) * EPS * (V @ aR)
    sp = f64(span)

    def d_sum(coef, dcoef):
        """unit of sum_j coef_j cf_j d_jc / span_c"""
        t = (coef * CF)[:, :, None] * D
        first = (dcoef * CF + coef * dcf)[:, :, None] * D + (coef * CF)[:, :, None] * dd
        return (first.sum(axis=1) + (n + 4) * EPS * t.sum(axis=1)) / sp

    dA = d_sum(np.broadcast_to(aal, (q, n)), np.zeros((q, n)))
    dB = d_sum(W, dw)
    return SimpleNamespace(q=q, k=k, n=n, vv=vv, mus=mus, A=A, B=B, dvv=dvv, dmus=dmus, dA=dA, dB=dB, v=v, dv=dv, xn=xn,
                           y_mean=float(gs["y_mean"]), y_std=float(gs["y_std"]), sq_min=f64(sq).min(axis=1))


def _posterior(lin, s2=None):
    """fp64 views of mean, unfloored variance (with the noise s2 where given), its unit and the floored sigma."""
    ym, ysd = lin.y_mean, lin.y_std
    mu = ym + ysd * f64(lin.mus)
    t = 1 - lin.vv
    dvar = ysd * ysd * (lin.dvv + EPS * (1.0 + 3.0 * np.abs(f64(t))))
    if s2 is not None:
        t = t + hp(s2)
        dvar = dvar + EPS * ysd * ysd * (s2 + np.abs(f64(t)))
    var = f64(t * (hp(ysd) * hp(ysd)))
    return mu, var, dvar, np.sqrt(np.maximum(var, FLOOR))


def near_floor(lin, s2=None):
    """Queries whose variance lies within VAR_MARGIN dvar of the floor: which side they fall on is rounding's choice."""
    _, var, dvar, _ = _posterior(lin, s2)
    return np.abs(var - FLOOR) <= VAR_MARGIN * dvar


# ---- the reference: scalar chain in mpmath -----------------------------------------------------------------------
def _mpf(x):
    """long double (or double) -> mpf, exactly."""
    x = hp(x)
    head = float(x)
    return MP.mpf(head) + MP.mpf(float(x - hp(head)))


def _ld(x):
    """mpf -> long double, to its precision."""
    head = float(x)
    return hp(head) + hp(float(x - MP.mpf(head)))


def _exact_helper(u):
    """phi, Phi, ei = phi + u Phi, h = log ei, h' = Phi / ei, h'' = phi / ei - h'^2 of an mpf u."""
    phi = MP.exp(-u * u / 2) / MP.sqrt(2 * MP.pi)
    Phi = MP.erfc(-u / MP.sqrt(2)) / 2
    ei = phi + u * Phi
    dh = Phi / ei
    return phi, Phi, ei, MP.log(ei), dh, phi / ei - dh * dh


def helper_units(u, du=0.0):
    """(h, h', h'', u_h, u_dh) of log_ei_helper at the double u, known to within du: the units of every branch that
    [u - du, u + du] reaches, the larger of them."""
    um = MP.mpf(u)
    phi, Phi, ei, h, dh, d2h = _exact_helper(um)
    au = abs(u)
    branches = set()
    for t in (u - du, u, u + du):
        branches.add(0 if t > -1.0 else (1 if t > -1e6 else 2))
    u_h = u_dh = 0.0
    if 0 in branches:
        dei = EPS * (float(phi) * (2.0 + u * u) + 3.0 * au * float(Phi) + float(ei))
        rel = float(MP.mpf(dei) / ei)
        u_h, u_dh = max(u_h, rel + EPS * abs(float(h))), max(u_dh, float(dh) * (3.0 * EPS + rel))
    if 1 in branches:
        x = -um / MP.sqrt(2)
        ex = MP.exp(x * x) * MP.erfc(x)
        E = ex * abs(um) * MP.sqrt(MP.pi / 2)
        one_m = 1 - E
        dw = um + MP.sqrt(2 / MP.pi) / ex + 1 / um
        r = float(E / one_m)
        u_h = max(u_h, 2.0 * EPS * (u * u / 2.0 + 1.0) + 4.0 * EPS * r + EPS * abs(float(MP.log(one_m))))
        u_dh = max(u_dh, EPS * au + 5.0 * EPS * au * r
                   + abs(float(dw)) * r * (4.0 * EPS + float((4.0 * EPS * E + EPS) / one_m) + 3.0 * EPS))
    if 2 in branches:
        u_h = max(u_h, 2.0 * EPS * (u * u / 2.0 + 2.0 * math.log(au) + 2.0))
        u_dh = max(u_dh, 2.0 * EPS * au)
    return h, dh, d2h, u_h, u_dh


def scalars(lin, best_f, maximize, acq):
    """Values and gradients of the acquisition at the queries of `lin` with their units (acq UCB: `best_f` is kappa)."""
    if acq == UCB:
        return scalars_ucb(lin, best_f, maximize)
    q, k = lin.q, lin.k
    ym, ysd, sgn = lin.y_mean, lin.y_std, (1.0 if maximize else -1.0)
    value, u_value = hp(np.zeros(q)), np.zeros(q)
    grad, u_grad = hp(np.zeros((q, k))), np.zeros((q, k))
    u_out, clamped_out = np.zeros(q), np.zeros(q, dtype=bool)
    aA, aB = np.abs(f64(lin.A)), np.abs(f64(lin.B))
    for i in range(q):
        mus, vv = _mpf(lin.mus[i]), _mpf(lin.vv[i])
        mu = MP.mpf(ym) + MP.mpf(ysd) * mus
        var = (1 - vv) * MP.mpf(ysd) * MP.mpf(ysd)
        clamped = not var >= MP.mpf(FLOOR)
        if clamped:
            var = MP.mpf(FLOOR)
        sigma = MP.sqrt(var)
        u = MP.mpf(sgn) * (mu - MP.mpf(best_f)) / sigma
        uf, sf = float(u), float(sigma)
        dmu = ysd * lin.dmus[i] + 2.0 * EPS * (abs(ym) + abs(ysd * float(mus)))
        dvar = ysd * ysd * (lin.dvv[i] + EPS * (1.0 + 3.0 * abs(float(1 - vv))))
        dsig = 0.0 if clamped else dvar / (2.0 * sf) + EPS * sf
        du = (dmu + EPS * abs(float(mu - MP.mpf(best_f)))) / sf + abs(uf) * dsig / sf + 2.0 * EPS * abs(uf)
        if acq == LOG_EI:
            _, _, _, u_h, u_dh = helper_units(uf, du)          # the units at the double nearest u,
            _, _, _, h, D, D2 = _exact_helper(u)               # the function at u itself
            val = h + MP.log(sigma)
            u_val = abs(float(D)) * du + u_h + dsig / sf + EPS * (abs(math.log(sf)) + abs(float(val)))
            dD = abs(float(D2)) * du + u_dh
            P = 1 / sigma
        else:
            phi, Phi = MP.exp(-u * u / 2) / MP.sqrt(2 * MP.pi), MP.erfc(-u / MP.sqrt(2)) / 2
            val, D = Phi, phi
            u_val = float(phi) * (du + 2.0 * EPS * abs(uf)) + 4.0 * EPS * float(Phi)
            dD = abs(uf) * float(phi) * du + EPS * float(phi) * (3.0 + uf * uf)
            P = MP.mpf(0)
        Df = abs(float(D))
        c_mu = D * MP.mpf(sgn) * MP.mpf(ysd) / sigma
        dc_mu = (ysd / sf) * (dD + Df * (dsig / sf + 3.0 * EPS))
        if clamped:
            c_sg, dc_sg = MP.mpf(0), 0.0
        else:
            T = P - D * u / sigma
            c_sg = T * (-(MP.mpf(ysd) * MP.mpf(ysd)) / sigma)
            dT = ((dsig / (sf * sf) + EPS / sf) if acq == LOG_EI else 0.0) \
                + (dD * abs(uf) + Df * du + Df * abs(uf) * (dsig / sf + 3.0 * EPS)) / sf + EPS * abs(float(T))
            dc_sg = (ysd * ysd / sf) * (dT + abs(float(T)) * (dsig / sf + 3.0 * EPS))
        cm, cs = _ld(c_mu), _ld(c_sg)
        value[i], u_value[i] = _ld(val), u_val
        grad[i] = cm * lin.A[i] + cs * lin.B[i]
        acm, acs = abs(float(cm)), abs(float(cs))
        u_grad[i] = acm * lin.dA[i] + aA[i] * dc_mu + acs * lin.dB[i] + aB[i] * dc_sg + 2.0 * EPS * (acm * aA[i] + acs * aB[i])
        u_out[i], clamped_out[i] = uf, clamped
    return SimpleNamespace(value=value, grad=grad, u_value=u_value, u_grad=u_grad, u=u_out, clamped=clamped_out)


def judge(ref, values, grads=None, rows=None):
    """(worst ratio of the values, worst ratio of the gradient components) of an implementation's results at the first
    len(values) queries of `ref` (or at `rows`); NaN and an error where the unit is 0 are infinite."""
    rows = slice(0, len(values)) if rows is None else rows
    rv = _ratio(hp(values) - ref.value[rows], ref.u_value[rows])
    rg = 0.0 if grads is None else _ratio(hp(grads) - ref.grad[rows], ref.u_grad[rows])
    return rv, rg


def well_conditioned(ref):
    """Queries at which two fp64 evaluations of log-EI's gradient can agree to 1e-10 whatever their summation order.
    In the middle branch of `log_ei_helper` each evaluation of h' carries 5 eps |u|^3 of rounding noise on |h'| ~ |u|
    (u_dh above), so two of them differ by up to 10 eps u^2 relative: at |u| <= 67 that is 1e-11, a tenth of the bound,
    the rest of which is left to the sums as everywhere else.  The tail branch (h' = -u - 2 / u, no cancellation)
    qualifies where u is decisively inside it.  From the reference's u alone."""
    return (np.abs(ref.u) <= 67.0) | (ref.u < -1e6 - 1.0)


def agreement(ref, g_a, g_b):
    """Worst |g_a - g_b| / u_grad over the components of two implementations' gradients at the first len(g_a) queries."""
    return _ratio(hp(g_a) - hp(g_b), ref.u_grad[:len(g_a)])


# ---- UCB and the posterior query: linear in the quantities of `linear()`, in long double ---------------------------
def scalars_ucb(lin, kappa, maximize):
    """`scalars()` for the upper confidence bound (same return shape; u is not defined and left 0)."""
    ym, ysd, sgn, kappa = lin.y_mean, lin.y_std, (1.0 if maximize else -1.0), float(kappa)
    mu = hp(ym) + hp(ysd) * lin.mus
    var = (1 - lin.vv) * (hp(ysd) * hp(ysd))
    clamped = ~(var >= hp(FLOOR))
    sigma = hp_sqrt(np.where(clamped, hp(FLOOR), var))
    sf = f64(sigma)
    dmu = ysd * lin.dmus + 2.0 * EPS * (abs(ym) + np.abs(ysd * f64(lin.mus)))
    dvar = ysd * ysd * (lin.dvv + EPS * (1.0 + 3.0 * np.abs(f64(1 - lin.vv))))
    dsig = np.where(clamped, 0.0, dvar / (2.0 * sf) + EPS * sf)
    value = hp(sgn) * mu + hp(kappa) * sigma
    u_value = dmu + kappa * dsig + EPS * (np.abs(kappa * sf) + np.abs(f64(value)))
    c_mu = hp(sgn) * hp(ysd)
    dc_mu = EPS * abs(sgn * ysd)
    c_sg = np.where(clamped, hp(0.0), -hp(kappa) * (hp(ysd) * hp(ysd)) / sigma)
    acs = np.abs(f64(c_sg))
    dc_sg = acs * (dsig / sf + 3.0 * EPS)                                     # 0 where clamped: c_sg is 0 there
    grad = c_mu * lin.A + c_sg[:, None] * lin.B
    aA, aB, acm = np.abs(f64(lin.A)), np.abs(f64(lin.B)), abs(sgn * ysd)
    u_grad = acm * lin.dA + aA * dc_mu + acs[:, None] * lin.dB + aB * dc_sg[:, None] \
        + 2.0 * EPS * (acm * aA + acs[:, None] * aB)
    return SimpleNamespace(value=value, grad=grad, u_value=u_value, u_grad=u_grad, u=np.zeros(lin.q), clamped=clamped)


def posterior(st, lin, noise=False):
    """Mean, floored variance and joint covariance of the posterior query at the queries of `lin`, with their units.
    The floored variance is exactly FLOOR (unit 0) where the raw one is below it; `check_posterior_conditions` sees to
    it that no raw variance is within rounding of the floor."""
    q, k, n, ls, s2 = lin.q, lin.k, lin.n, float(st.lengthscale), float(st.noise)
    ym, ysd = lin.y_mean, lin.y_std
    ys2 = hp(ysd) * hp(ysd)
    mean = hp(ym) + hp(ysd) * lin.mus
    u_mean = ysd * lin.dmus + 2.0 * EPS * (abs(ym) + np.abs(ysd * f64(lin.mus)))
    t = 1 - lin.vv
    u_raw = ysd * ysd * (lin.dvv + EPS * (1.0 + 3.0 * np.abs(f64(t))))
    if noise:
        t = t + hp(s2)
        u_raw = u_raw + EPS * ysd * ysd * (s2 + np.abs(f64(t)))
    raw = t * ys2
    clamped = ~(raw >= hp(FLOOR))
    var, u_var = np.where(clamped, hp(FLOOR), raw), np.where(clamped, 0.0, u_raw)
    xn = lin.xn
    d = xn[:, None, :] - xn[None, :, :]                                         # q x q x k
    ssq = (d * d).sum(axis=2)
    sq = ssq / (hp(ls) * hp(ls))
    kq, _, dkq_dsq, _, arg = _cov(sq, st.kernel, ls)
    vab = lin.v @ lin.v.T
    core = kq - vab
    cov = ys2 * core
    D, XN, V = np.abs(f64(d)), np.abs(f64(xn)), np.abs(f64(lin.v))
    dd = 2.0 * EPS * (XN[:, None, :] + XN[None, :, :]) + EPS * D
    dsq = (2.0 * (D * dd).sum(axis=2) + (k + 2) * EPS * f64(ssq)) / (ls * ls) + 3.0 * EPS * f64(sq)
    dkq = f64(dkq_dsq) * dsq + EPS * np.abs(f64(kq)) * (4.0 + f64(arg))
    dvab = V @ lin.dv.T + lin.dv @ V.T + (n + 2) * EPS * (V @ V.T)
    u_cov = ysd * ysd * (dkq + dvab + EPS * np.abs(f64(core))) + 3.0 * EPS * np.abs(f64(cov))
    i = np.arange(q)
    cov[i, i], u_cov[i, i] = raw, u_raw                                         # the diagonal: the raw variance
    return SimpleNamespace(mean=mean, u_mean=u_mean, variance=var, u_variance=u_var, raw=raw, u_raw=u_raw,
                           covariance=cov, u_covariance=u_cov, clamped=clamped)


def judge_posterior(ref, out):
    """{mean, variance[, covariance]: worst ratio} of an implementation's posterior at the first len(mean) queries."""
    q = len(out["mean"])
    r = {"mean": _ratio(hp(out["mean"]) - ref.mean[:q], ref.u_mean[:q]),
         "variance": _ratio(hp(out["variance"]) - ref.variance[:q], ref.u_variance[:q])}
    if out.get("covariance") is not None:
        r["covariance"] = _ratio(hp(out["covariance"]) - ref.covariance[:q, :q], ref.u_covariance[:q, :q])
    return r


# ---- references on a device's own state, shared by the device test files -----------------------------------------
_REFS = {}


def digest(gs):
    h = hashlib.sha256()
    for key in ("R", "alpha", "norm_bounds"):
        h.update(np.ascontiguousarray(gs[key], dtype=np.float64).tobytes())
    h.update(np.array([gs["y_mean"], gs["y_std"]], dtype=np.float64).tobytes())
    return h.hexdigest()


def cached_linear(st, gs):
    """(key, linear part of the reference) on a conditioned state, once per distinct state (objects that hold the
    same bits share it) and never modified."""
    key = (st.name, digest(gs))
    if key not in _REFS:
        _REFS[key] = {"lin": linear(st, gs, st.X)}
    return key, _REFS[key]["lin"]


def cached_scalars(key, label, acq, mx, best):
    """Reference of one scalar on one conditioned state, cached per (state, scalar)."""
    if label not in _REFS[key]:
        _REFS[key][label] = scalars(_REFS[key]["lin"], best, mx, acq)
    return _REFS[key][label]


def cached_posterior(st, key, noise):
    label = ("posterior", bool(noise))
    if label not in _REFS[key]:
        _REFS[key][label] = posterior(st, _REFS[key]["lin"], noise)
    return _REFS[key][label]


# ---- the scalars of a state --------------------------------------------------------------------------------------
def cases(lin):
    """[(label, acq, maximize, best_f)]: per direction log-EI at `near`, `mid` (50 s_y away) and `far` (1e9 s_y) as
    tools/gpu_acq_paths_hashes.py chooses them, log-EI at three seam incumbents that put the u of query SEAM_QUERY at
    -1, -1 - 1e-6 and -1e6 to rounding, and PI at `near` and `3sigma`."""
    mu, _, _, sigma = _posterior(lin)
    ym, ysd = lin.y_mean, lin.y_std
    out = []
    for maximize in (0, 1):
        sgn = 1.0 if maximize else -1.0
        near = float(np.median(mu[:32]))
        inc = {"near": near, "3sigma": float(near + sgn * 3.0 * np.median(sigma[:32])),
               "mid": float(ym + sgn * 50.0 * ysd), "far": float(ym + sgn * 1e9 * ysd)}
        for tag, t in (("seam-1", -1.0), ("seam-1-1e-6", -1.0 - 1e-6), ("seam-1e6", -1e6)):
            inc[tag] = float(mu[SEAM_QUERY] - sgn * t * sigma[SEAM_QUERY])        # u = sgn (mu - best) / sigma = t
        out += [("log_ei,%d,%s" % (maximize, t), LOG_EI, maximize, inc[t])
                for t in ("near", "mid", "far", "seam-1", "seam-1-1e-6", "seam-1e6")]
        out += [("pi,%d,%s" % (maximize, t), PI, maximize, inc[t]) for t in ("near", "3sigma")]
    return out


def u_of(lin, best_f, maximize):
    """u of every query in fp64 (for the conditions; the judged u is that of `scalars`)."""
    mu, _, _, sigma = _posterior(lin)
    return (1.0 if maximize else -1.0) * (mu - best_f) / sigma


def cases_ucb(lin=None):
    """[(label, UCB, maximize, kappa)]: every kappa of KAPPAS in both directions."""
    return [("ucb,%d,%s" % (mx, ("%.3g" % kap)), UCB, mx, kap) for mx in (0, 1) for kap in KAPPAS]


def _state_conditions(name, st, lin):
    """The conditions on the queries and the variances, whatever is evaluated there."""
    bad = []
    X, Z = st.X, st.Z
    if not (np.array_equal(X[0], Z[0]) and np.array_equal(X[1], Z[1]) and np.array_equal(X[3], X[4])):
        bad.append("the hand-placed queries are not in place")
    if not (lin.sq_min[0] == 0.0 and lin.sq_min[1] == 0.0 and 0.0 < lin.sq_min[2] < 1e-12):
        bad.append(("sq of the training-point queries", lin.sq_min[:3]))
    if near_floor(lin).any():
        bad.append(("variance within %g dvar of the floor" % VAR_MARGIN, np.flatnonzero(near_floor(lin))))
    _, var, _, _ = _posterior(lin)
    cl = var[:32] < FLOOR
    if name == "E" and not cl.all():
        bad.append("state E has free variances")
    if name == "mixed" and not (cl.sum() >= 4 and (~cl).sum() >= 4 and cl[:5].any() and (~cl[:5]).any()):
        bad.append(("state mixed is not mixed", int(cl.sum())))
    if name not in ("E", "mixed") and cl.any():
        bad.append("a clamped variance outside E and mixed")
    return bad


def check_ucb_conditions(name, st, lin):
    """What the device test of UCB relies on, as a list of violations (empty: all hold).  UCB has no u and no
    branches: the conditions are those on the queries and on the floor."""
    return _state_conditions(name, st, lin)


def check_posterior_conditions(name, st, lin):
    """What the device test of the posterior query relies on: the conditions on the queries and the floor, no variance
    WITH the observation noise within rounding of the floor either, and the near-coincident pairs in place (1e-9 apart
    per coordinate: a scaled squared distance above 0 and below 1e-12)."""
    bad = _state_conditions(name, st, lin)
    if near_floor(lin, st.noise).any():
        bad.append(("noisy variance within %g dvar of the floor" % VAR_MARGIN, np.flatnonzero(near_floor(lin, st.noise))))
    ls2 = float(st.lengthscale) ** 2
    for a, b in NEAR_PAIRS:
        sq = float(((lin.xn[a] - lin.xn[b]) ** 2).sum()) / ls2
        if not (np.array_equal(st.X[b], st.X[a] + 1e-9) and 0.0 < sq < 1e-12):
            bad.append(("near-coincident pair", a, b, sq))
    if not float(((lin.xn[3] - lin.xn[4]) ** 2).sum()) == 0.0:
        bad.append("the duplicate pair is not one")
    return bad


def check_conditions(name, st, lin):
    """What the device test relies on, as a list of violations (empty: all hold)."""
    bad = _state_conditions(name, st, lin)
    for label, _, maximize, best_f in cases(lin):
        u, tag = u_of(lin, best_f, maximize)[:32], label.split(",")[2]
        ok = {"near": (u > -0.5).any(), "mid": ((u < -2.0) & (u > -1e5)).all(), "far": (u < -1e7).all(),
              "3sigma": ((u < -1.0) & (u > -6.0)).any(), "seam-1": abs(u[SEAM_QUERY] + 1.0) < 1e-9,
              "seam-1-1e-6": abs(u[SEAM_QUERY] + 1.0 + 1e-6) < 1e-9 and u[SEAM_QUERY] < -1.0,
              "seam-1e6": abs(u[SEAM_QUERY] + 1e6) < 1e-3}[tag]
        if not ok:
            bad.append((label, "u does not reach its branch", float(u[SEAM_QUERY])))
    return bad


# ---- the chain in plain fp64, as the kernels write it -------------------------------------------------------------
def helper_restated(u, sqrt_pi_2=1.2533141373155003, tail_from=None):
    """`log_ei_helper` of acq_math.h on a numpy array, through scipy's erfcx / erfc / log1p: (h, h').  Wrong variants:
    sqrt(pi / 2) truncated; the tail asymptote taken for tail_from < u < -1 as well."""
    from scipy.special import erfc, erfcx
    u = np.asarray(u, dtype=np.float64)
    h, dh = np.empty_like(u), np.empty_like(u)
    with np.errstate(all="ignore"):
        up = u > -1.0
        tail = u <= -1e6
        if tail_from is not None:
            tail = tail | ((u > tail_from) & (u <= -1.0))
        mid = ~up & ~tail
        x = u[up]
        phi = 0.3989422804014327 * np.exp(-0.5 * x * x)
        Phi = 0.5 * erfc(-0.7071067811865476 * x)
        ei = phi + x * Phi
        h[up], dh[up] = np.log(ei), Phi / ei
        x = u[mid]
        log_phi = -0.5 * (x * x + 1.8378770664093453)
        ex = erfcx(-0.7071067811865476 * x)
        E = (ex * np.abs(x)) * sqrt_pi_2
        dw = (x + 0.7978845608028654 / ex) + 1.0 / x
        h[mid], dh[mid] = log_phi + np.log1p(-E), -x - dw * E / (1.0 - E)
        x = u[tail]
        h[tail], dh[tail] = -0.5 * (x * x + 1.8378770664093453) - 2.0 * np.log(np.abs(x)), -x - 2.0 / x
    return h, dh


def restate(st, gs, X, best_f, maximize, acq, coef53=5.0 / 3.0, drop_last_v=False, sqrt_pi_2=1.2533141373155003,
            cmu_unsigned=False, csg_keep_clamped=False, tail_from=None, pi_grad_Phi=False):
    """numpy fp64 restatement of the chain: direct distance, R @ ks, the three branches of `log_ei_helper`.  Each
    keyword switches on one wrong variant: the 5/3 of the Matern radial factor (pass a float32), the last row of v left
    out of |v|^2, sqrt(pi / 2) truncated in the middle branch, c_mu without its sign, c_sg not zeroed at a clamped
    variance, the tail asymptote in tail_from < u < -1, PI's gradient with Phi in place of phi."""
    from scipy.special import erfc
    X = np.asarray(X, dtype=np.float64)
    R, alpha = np.tril(gs["R"]), np.asarray(gs["alpha"], dtype=np.float64)
    lo, hi = gs["norm_bounds"][0], gs["norm_bounds"][1]
    ym, ysd, ls = float(gs["y_mean"]), float(gs["y_std"]), float(st.lengthscale)
    xn, zn = (X - lo) / (hi - lo), (st.Z - lo) / (hi - lo)
    d = xn[:, None, :] - zn[None, :, :]
    sq = (d * d).sum(axis=2) * ((1.0 / ls) * (1.0 / ls))
    if st.kernel == "rbf":
        ks = np.exp(-0.5 * sq)
        rf = -ks
    else:
        dist = np.sqrt(np.maximum(sq, 1e-30))
        e = np.exp(-_S5 * dist)
        ks = ((_S5 * dist + 1.0) + (5.0 / 3.0) * (dist * dist)) * e
        rf = -float(coef53) * (1.0 + _S5 * dist) * e
    cf = rf * (1.0 / ls) * (1.0 / ls)
    v = ks @ R.T
    vv = (v[:, :-1] * v[:, :-1]).sum(axis=1) if drop_last_v else (v * v).sum(axis=1)
    mus = ks @ alpha
    w = v @ R
    gm = np.einsum("qj,qjc->qc", alpha[None, :] * cf, d)
    gs_ = np.einsum("qj,qjc->qc", w * cf, d)
    mu = ym + ysd * mus
    var = (1.0 - vv) * (ysd * ysd)
    clamped = ~(var >= FLOOR)
    sigma = np.sqrt(np.where(clamped, FLOOR, var))
    sgn = 1.0 if maximize else -1.0
    if acq == UCB:                       # kappa in the best_f slot; the kernels' one fused multiply-add as two roundings
        kappa = float(best_f)
        c_sg = kappa * (-(ysd * ysd) / sigma)
        if not csg_keep_clamped:
            c_sg = np.where(clamped, 0.0, c_sg)
        return kappa * sigma + sgn * mu, ((sgn * ysd) * gm + c_sg[:, None] * gs_) / (hi - lo)
    u = (mu - best_f) / sigma * sgn
    with np.errstate(all="ignore"):
        if acq == LOG_EI:
            h, dv_du = helper_restated(u, sqrt_pi_2, tail_from)
            val, dv_dsig = h + np.log(sigma), 1.0 / sigma
        else:
            val = 0.5 * erfc(-0.7071067811865476 * u)
            dv_du = val if pi_grad_Phi else 0.3989422804014327 * np.exp(-0.5 * u * u)
            dv_dsig = 0.0
        c_mu = dv_du * (1.0 if cmu_unsigned else sgn) * ysd / sigma
        c_sg = (dv_dsig - dv_du * u / sigma) * (-(ysd * ysd) / sigma)
        if not csg_keep_clamped:
            c_sg = np.where(clamped, 0.0, c_sg)
        grad = (c_mu[:, None] * gm + c_sg[:, None] * gs_) / (hi - lo)
    return val, grad


def _float32_strength(ref):
    """A wrong 5/3 scales cf, and with it every gradient, by 1 + rho exactly: the variant stands rho |g| / u_grad above the
    reference, no more.  The largest such ratio over the queries, from reference quantities alone."""
    rho = abs(float(np.float32(5.0 / 3.0)) / (5.0 / 3.0) - 1.0)
    pos = ref.u_grad > 0.0
    return float((rho * np.abs(f64(ref.grad))[pos] / ref.u_grad[pos]).max())


# variant -> (keyword arguments of restate, what it damages, which cases it applies to[, the strength at which the
# reference itself says the variant can be seen])
# "tail asymptote in -1.5 < u < -1" stands for the issue's "wrong branch taken in -1.5 < u < -1".  Swapping the two
# ACCURATE formulas of log_ei_helper there is no error: either is within its unit on both sides of u = -1 (at u = -1.3
# the direct form loses a factor 4 to the cancellation of phi + u Phi, the erfcx form as much to E / (1 - E) = 2.8),
# which is what the seam rule - the larger unit of the two branches - expresses, so no unit can or should see it.  The
# only branch that is wrong there is the tail's: a gross error (1e10 units), which shows that a misplaced branch is
# seen, not how sharp the units are at the seam - that is shown by the truncated sqrt(pi / 2).
WRONG = {
    "5/3 of the radial factor as a float32": (dict(coef53=np.float32(5.0 / 3.0)), "grad",
                                              lambda st, label, ref: st.kernel != "rbf", _float32_strength),
    "last row of v left out of |v|^2": (dict(drop_last_v=True), "any", lambda st, label, ref: not ref.clamped.all()),
    "sqrt(pi/2) truncated to 8 digits": (dict(sqrt_pi_2=1.2533141), "value",
                                         lambda st, label, ref: label.startswith("log_ei") and label.endswith("mid")),
    "c_mu without its sign": (dict(cmu_unsigned=True), "grad", lambda st, label, ref: label.split(",")[1] == "0"),
    "c_sg kept at a clamped variance": (dict(csg_keep_clamped=True), "grad", lambda st, label, ref: ref.clamped.any()),
    "tail asymptote in -1.5 < u < -1": (dict(tail_from=-1.5), "value",
                                        lambda st, label, ref: label.startswith("log_ei") and "seam-1-1e-6" in label),
    "PI's gradient with Phi for phi": (dict(pi_grad_Phi=True), "grad", lambda st, label, ref: label.startswith("pi")),
}


# ---- UCB and the posterior query in plain fp64 --------------------------------------------------------------------
# UCB goes through `restate` (acq = UCB).  variant -> (keyword arguments of restate, what it damages, the kappas it can
# be seen at, the states on which it must leave the device's limit)
WRONG_UCB = {
    "5/3 of the radial factor as a float32": (dict(coef53=np.float32(5.0 / 3.0)), "grad", KAPPAS, ("B", "D", "k128", "n385k65")),
    "last row of v left out of |v|^2": (dict(drop_last_v=True), "any", KAPPAS[1:], ("A", "B", "B-rbf", "user", "n385k65")),
    "c_sg kept at a clamped variance": (dict(csg_keep_clamped=True), "grad", KAPPAS[1:], ("E", "mixed")),
}


def _ks64(sq, kernel, coef53=5.0 / 3.0):
    """The covariance of acq_math.h's `acq_cov` on an fp64 array of scaled squared distances."""
    if kernel == "rbf":
        return np.exp(-0.5 * sq)
    dist = np.sqrt(np.maximum(sq, 1e-30))
    return ((_S5 * dist + 1.0) + float(coef53) * (dist * dist)) * np.exp(-_S5 * dist)


def restate_posterior(st, gs, X, noise=False, coef53=5.0 / 3.0, drop_last_v=False, qq_norms=False, diag_from_tile=False,
                      floor_diag=False, noise_after=False):
    """numpy fp64 restatement of the posterior query as kernels_post.hip writes it: direct distances, the 1e-30 guard,
    V = R KS^T, the variance from the column norms of V, the covariance (k(Xq, Xq) - V^T V) s_y^2 with the raw variance
    on its diagonal.  Each keyword switches on one wrong variant: the 5/3 of the Matern polynomial as a float32, the
    last row of V dropped, the query-query distance as |a|^2 + |b|^2 - 2 a.b, the covariance's diagonal from the tile
    product (whose epilogue knows no noise), the floor applied to that diagonal, the noise added after the
    multiplication by s_y^2."""
    X = np.asarray(X, dtype=np.float64)
    R, alpha = np.tril(gs["R"]), np.asarray(gs["alpha"], dtype=np.float64)
    lo, hi = gs["norm_bounds"][0], gs["norm_bounds"][1]
    ym, ysd, ls, s2 = float(gs["y_mean"]), float(gs["y_std"]), float(st.lengthscale), float(st.noise)
    il2 = (1.0 / ls) * (1.0 / ls)
    xn, zn = (X - lo) / (hi - lo), (st.Z - lo) / (hi - lo)
    d = xn[:, None, :] - zn[None, :, :]
    ks = _ks64((d * d).sum(axis=2) * il2, st.kernel, coef53)
    V = R @ ks.T                                                               # n x q
    if drop_last_v:
        V = V[:-1]
    vv = (V * V).sum(axis=0)
    mean = ym + ysd * (ks @ alpha)
    if noise_after:
        raw = (1.0 - vv) * (ysd * ysd) + (s2 if noise else 0.0)
    else:
        raw = ((1.0 - vv) + s2) * (ysd * ysd) if noise else (1.0 - vv) * (ysd * ysd)
    var = np.where(raw >= FLOOR, raw, FLOOR)
    if qq_norms:
        # elementwise numpy only, so that every machine rounds alike: the norms summed over the coordinates in
        # ascending order, the dot products as a tile product would chain them, four coordinates per step
        kk = xn.shape[1]
        nrm, dot = np.zeros(len(X)), np.zeros((len(X), len(X)))
        prod = [xn[:, c, None] * xn[None, :, c] for c in range(kk)] + [np.zeros((len(X), len(X)))] * (-kk % 4)
        for c in range(kk):
            nrm = nrm + xn[:, c] * xn[:, c]
        for c in range(0, kk, 4):
            dot = dot + ((prod[c] + prod[c + 1]) + (prod[c + 2] + prod[c + 3]))
        sqq = np.maximum((nrm[:, None] + nrm[None, :]) - 2.0 * dot, 0.0) * il2
    else:
        dq = xn[:, None, :] - xn[None, :, :]
        sqq = (dq * dq).sum(axis=2) * il2
    cov = (_ks64(sqq, st.kernel, coef53) - V.T @ V) * (ysd * ysd)
    if not diag_from_tile:
        i = np.arange(len(X))
        cov[i, i] = var if floor_diag else raw
    return {"mean": mean, "variance": var, "covariance": cov}


# variant -> (keyword arguments of restate_posterior, the noise flags it can be seen under, the states on which it must
# leave the device's limit)
WRONG_POSTERIOR = {
    "5/3 of the Matern polynomial as a float32": (dict(coef53=np.float32(5.0 / 3.0)), (False, True), ("A", "B", "D", "n64", "n385k65")),
    "last row of v dropped": (dict(drop_last_v=True), (False, True), ("A", "B", "B-rbf", "user", "n385k65")),
    "query-query distance as norms minus a dot product": (dict(qq_norms=True), (False, True), ("k128",)),
    "covariance diagonal from the tile product": (dict(diag_from_tile=True), (True,), ("A", "B", "B-rbf", "user", "E", "n385k65")),
    "floor applied to the covariance diagonal": (dict(floor_diag=True), (False, True), ("E", "mixed")),
    "noise added after the multiplication by y_std^2": (dict(noise_after=True), (True,), ("A", "B", "user", "mixed", "n385k65")),
}
