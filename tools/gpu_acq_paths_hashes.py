"""sha256 of what every acquisition path returns, for all three acquisitions in both directions, on seeded GP states: the golden
hash files of k_acq_fast and k_acq_group pin log-EI with the Matern kernel only, this one pins the rest of the scalar maths that
the paths share (acq_math.h: covariance, log-EI / PI / UCB chain) - RBF, PI, UCB, maximize, the clamped variance, the tail
branches of log-EI - on every path that evaluates it:
  ctx_q32 / ctx_q40      acq_eval: per-query kernels with the in-launch finish / with partial records + k_acq_combine
  ctx_q512_tail{1,0}     gp_wait_eval: GEMM scoring, on two streams (PCABO_OPT_HIDDEN_TAIL = 1, k_score_ks_only) and on one
  grp_*                  the same on a PCABO_OPT_GROUP_ACQ context (k_acq_group)
  batch_q512             Batch.gp_wait_eval: the batched scoring launch
  device_q32             Batch(device_lbfgsb=1).device_acq_eval: lb_eval of the device-resident optimiser (k <= 40)
The states are the smallest shapes that reach each code form (tests/test_gpu_ucb.py), plus the state of
test_log_ei_tail_branches.  The scalars (incumbent / kappa) are chosen from a float64 numpy posterior of this file's own so that
the hashed queries reach every branch of the chain: u > -1, -1e6 < u <= -1, u <= -1e6 and a clamped variance (cases() asserts
it; it needs no GPU), and PI is evaluated where it is not 0.  tests/golden/acq_paths_hashes.json holds the bits of the library
before the scalar maths moved into acq_math.h (PCABO_LIB selects the library).
    python tools/gpu_acq_paths_hashes.py            # print
    python tools/gpu_acq_paths_hashes.py --write    # regenerate (only after an INTENDED change of arithmetic)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "acq_paths_hashes.json")
LENGTHSCALE, NOISE = 0.6931471805599453, 0.006737946999085467      # the defaults of gp_condition
# state -> (n, k, scale of y, kernel)
STATES = {
    "A": (9, 1, 1.0, "matern52"),          # k_acq_fast, NP = 64, one component
    "B": (70, 6, 1.0, "matern52"),         # k_acq_fast, NP = 128, 16-row slabs
    "B-rbf": (70, 6, 1.0, "rbf"),
    "C": (449, 10, 1.0, "matern52"),       # k_acq_fast, NP = 512, 32-row slabs; lb_eval with 2 row parts
    "D": (50, 41, 1.0, "matern52"),        # k_acq_fused (k > 40); no device optimiser
    "E": (30, 3, 1e-7, "matern52"),        # every query's variance under the 1e-10 floor
    "T": (64, 3, 1.0, "matern52"),         # the inputs of test_log_ei_tail_branches
}
LOG_EI, PI, UCB = 0, 1, 2
Q = 512                                    # queries per state; every path takes a prefix, all of them the first 32


def make_state(name):
    """(Z, y, kernel, X): training points, values and the Q query points of a state."""
    n, k, yscale, kernel = STATES[name]
    if name == "T":
        rng = np.random.default_rng(3)
        Z = rng.uniform(-1, 1, size=(n, k))
        y = rng.normal(size=n)
        return Z, y, kernel, rng.uniform(-1, 1, size=(Q, k))
    rng = np.random.default_rng(1000 + 10 * n + k)
    Z = rng.normal(size=(n, k))
    y = (rng.normal(size=n) * 30.0 + 200.0) * yscale
    zmin, span = Z.min(0), Z.max(0) - Z.min(0)
    X = np.vstack([rng.uniform(zmin - 0.5 * span, zmin + 1.5 * span, size=(Q - 2, k)), Z[:2]])   # the search box + two training points
    X[30:32], X[38:40] = Z[:2], Z[:2]                                                            # (in every prefix the paths take)
    return Z, y, kernel, X


def posterior(Z, y, kernel, X):
    """float64 numpy posterior of the un-trained model: (mean[q], unclamped variance[q]) un-standardised."""
    zmin, span = Z.min(0), Z.max(0) - Z.min(0)
    lo, hi = zmin - 0.1 * span, zmin + 1.1 * span

    def cov(a, b):
        sq = (((a[:, None, :] - b[None, :, :]) / LENGTHSCALE) ** 2).sum(-1)
        if kernel == "rbf":
            return np.exp(-0.5 * sq)
        d = np.sqrt(np.maximum(sq, 1e-30))
        return (1.0 + np.sqrt(5.0) * d + 5.0 / 3.0 * d * d) * np.exp(-np.sqrt(5.0) * d)
    zn, xn = (Z - lo) / (hi - lo), (X - lo) / (hi - lo)
    ym, ysd = y.mean(), y.std(ddof=1)
    L = np.linalg.cholesky(cov(zn, zn) + NOISE * np.eye(len(y)))
    ks = cov(xn, zn)
    v = np.linalg.solve(L, ks.T)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, (y - ym) / ysd))
    return ym + ysd * (ks @ alpha), (1.0 - (v * v).sum(0)) * ysd * ysd


def chain_inputs(name):
    """(mu[32], sigma[32], clamped[32]) of the 32 queries every path shares, from posterior(): what the scalar chain starts from."""
    Z, y, kernel, X = make_state(name)
    mu, var = posterior(Z, y, kernel, X[:32])
    return mu, np.sqrt(np.maximum(var, 1e-10)), var < 1e-10


def incumbents(name, maximize):
    """The incumbents of a state and direction: near the posterior means, a few sigma, 50 and 1e9 standard deviations of y on the
    losing side of them."""
    _, y, _, _ = make_state(name)
    mu, sigma, _ = chain_inputs(name)
    ym, ysd, sgn = y.mean(), y.std(ddof=1), (1.0 if maximize else -1.0)
    return {"near": float(np.median(mu)), "3sigma": float(np.median(mu) + sgn * 3.0 * np.median(sigma)),
            "mid": float(ym + sgn * 50.0 * ysd), "far": float(ym + sgn * 1e9 * ysd)}


def u_of(name, maximize, best):
    mu, sigma, _ = chain_inputs(name)
    return (1.0 if maximize else -1.0) * (mu - best) / sigma


def cases(name):
    """[(label, acq, maximize, scalar)] of a state: log-EI at three incumbents (near, mid, far), PI at two (near, 3sigma: PI is
    exactly 0 further out), UCB at beta = 2 and 0.25.  Asserts that the first 32 queries reach the branches of the chain that the
    incumbents are meant for, with margins that rounding cannot cross."""
    _, _, clamped = chain_inputs(name)
    assert clamped.all() if name == "E" else not clamped.any(), name
    out = []
    for maximize in (0, 1):
        inc = incumbents(name, maximize)
        u = {k: u_of(name, maximize, v) for k, v in inc.items()}
        assert (u["near"] > -0.5).any(), (name, maximize)                                        # u > -1
        assert ((u["mid"] < -2.0) & (u["mid"] > -1e5)).all(), (name, maximize)                  # -1e6 < u <= -1
        assert (u["far"] < -1e7).all(), (name, maximize)                                         # u <= -1e6
        assert ((u["3sigma"] < -1.0) & (u["3sigma"] > -6.0)).any(), (name, maximize)             # PI between 1e-9 and 0.16: not 0
        out += [("log_ei,%d,%s" % (maximize, k), LOG_EI, maximize, inc[k]) for k in ("near", "mid", "far")]
        out += [("pi,%d,%s" % (maximize, k), PI, maximize, inc[k]) for k in ("near", "3sigma")]
        out += [("ucb,%d,beta%g" % (maximize, beta), UCB, maximize, float(np.sqrt(np.float32(beta)))) for beta in (2.0, 0.25)]
    return out


def _h(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        assert np.isfinite(a).all()
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def compute_state(name) -> dict:
    from pcabo import _native as N
    n, k, _, kernel = STATES[name]
    Z, y, _, X = make_state(name)
    kcode = N.KERNEL_RBF if kernel == "rbf" else N.KERNEL_MATERN52
    ctx = N.Context(max_n=n, max_d=k, max_q=Q)
    grp = N.Context(max_n=n, max_d=k, max_q=Q)
    grp.set_option(N.OPT_GROUP_ACQ, 1)
    on_device = k <= 40                                                      # the device optimiser's limit
    bt = N.Batch(1, max_n=n, max_d=k, max_q=Q, device_lbfgsb=1 if on_device else 0)
    out = {}
    for label, acq, maximize, scalar in cases(name):
        rec = {}
        for tag, c in (("ctx", ctx), ("grp", grp)):
            c.gp_condition(y, Z=Z, kernel=kcode)
            rec[tag + "_q32"] = _h(*c.acq_eval(X[:32], scalar, maximize, acq))
            rec[tag + "_q40"] = _h(*c.acq_eval(X[:40], scalar, maximize, acq))
            for tail in (1, 0):
                c.set_option(N.OPT_HIDDEN_TAIL, tail)
                c.gp_condition(y, Z=Z, kernel=kcode, wait=False)
                rec["%s_q512_tail%d" % (tag, tail)] = _h(c.gp_wait_eval(X, scalar, maximize, acq))
            c.set_option(N.OPT_HIDDEN_TAIL, 1)
        bt.gp_condition_begin(Z[None], y[None], kernel=kcode)
        vb, st = bt.gp_wait_eval([X], [scalar], maximize, acq)
        assert not st.any()
        rec["batch_q512"] = _h(vb[0])
        if on_device:
            vd, gd = bt.device_acq_eval([X[:32]], [scalar], maximize, acq)
            rec["device_q32"] = _h(vd[0], gd[0])
        out[label] = rec
    ctx.close(); grp.close(); bt.close()
    return out


def compute() -> dict:
    return {name: compute_state(name) for name in STATES}


if __name__ == "__main__":
    res = compute()
    if "--write" in sys.argv:
        i = sys.argv.index("--write")
        out = sys.argv[i + 1] if len(sys.argv) > i + 1 else GOLDEN
        with open(out, "w") as f:
            json.dump({"_comment": "tools/gpu_acq_paths_hashes.py --write on an MI355X, with the library as it was before the "
                                   "scalar maths of the acquisition moved into acq_math.h", "cases": res}, f, indent=1)
        print("written", out)
    else:
        print(json.dumps(res, indent=1))
