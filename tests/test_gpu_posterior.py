"""GP posterior queries on the MI355X (pcabo_gp_posterior / pcabo_batch_gp_posterior: k_score_ks, k_score_gemm, k_post_combine,
k_post_cov; Context.gp_posterior, Batch.gp_posterior, PCA_BO.posterior, Vanilla_BO.posterior) against tests/posterior_reference.py.

Shapes (n, k, q) of CASES: n crosses one R block (9), an exact block (64), two blocks (65, 130), two 256-column blocks of k_score_ks
(257), a late size (449) and the generic sizes (1050, 89); k crosses the 8-wide coordinate loop (1, 3, 8, 9) and the fast path's 40
(41, 89); q crosses the 16-query blocks of score_ks_block (1, 15, 16, 17), one partial / exact / exact-plus-one covariance tile (63,
64, 65) and three tiles with off-diagonal ones and a partial last one (130).  Every case asks for the covariance; Matern and RBF,
both noise flags, data-derived and user-supplied Normalize bounds all appear.  One more state is a late one of
tests/golden/late_state_d40.npz.

Error units: mean |d| / max(1, |mean|); variance and covariance |d| / s_y^2 (the prior variance, the scale of the cancellation
1 - |v|^2).  Tolerances: 10 x the largest error measured against the reference on an MI355X over CASES, the late state and the two
fitted states (the first test prints the worst ratios; EXPERIMENTS.md "GP posterior queries" has them per shape).
tests/test_gpu_posterior_edges.py judges the same kernels in derived fp64 error units, every covariance entry in its own.
"""
import os

import numpy as np
import pytest
import torch

import pcabo_oracle as O
from ard_reference import ard_state, fitted_gp
from pcabo.bbob import BBOBProblem
from posterior_reference import posterior, scalar_fit_as_ard
from ucb_reference import bbob_state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "late_state_d40.npz")
# 10 x the measured maxima: mean 4.79e-13, variance 1.27e-14, covariance 1.27e-14, all three at the late state (420, 8, 130)
TOL_MEAN, TOL_VAR, TOL_COV = 4.8e-12, 1.3e-13, 1.3e-13
# (n, k, q, kernel, observation noise, user-supplied Normalize bounds)
CASES = [(9, 1, 1, "matern52", False, False), (64, 3, 15, "rbf", True, True), (65, 8, 16, "matern52", False, True),
         (130, 9, 17, "matern52", True, False), (257, 41, 63, "rbf", False, False), (130, 3, 64, "matern52", False, False),
         (65, 9, 65, "rbf", True, True), (257, 8, 130, "matern52", True, False), (449, 41, 64, "matern52", False, True),
         (1050, 89, 65, "matern52", True, False)]
KERNEL = {"matern52": 0, "rbf": 1}


def _queries(Z, q, seed):
    """q points around the data; where there is room, two that almost coincide and one that is a training point."""
    rng = np.random.default_rng(seed)
    lo, hi = Z.min(0), Z.max(0)
    X = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), size=(q, Z.shape[1]))
    if q >= 3:
        X[1] = X[0] + 1e-9
        X[2] = Z[0]
    return X


def _errors(out, ref):
    sy2 = ref["y_std"] ** 2
    em = float((np.abs(out["mean"] - ref["mean"]) / np.maximum(1.0, np.abs(ref["mean"]))).max())
    ev = float(np.abs(out["variance"] - ref["variance"]).max() / sy2)
    ec = float(np.abs(out["covariance"] - ref["covariance"]).max() / sy2)
    return em, ev, ec


def _assert_close(out, ref, what):
    em, ev, ec = _errors(out, ref)
    print(f"  {what}: mean {em:.2e}, variance {ev:.2e}, covariance {ec:.2e}")
    assert em <= TOL_MEAN and ev <= TOL_VAR and ec <= TOL_COV, (what, em, ev, ec)
    return em, ev, ec


@pytest.fixture(scope="module")
def ctx(native):
    torch.set_num_threads(8)
    c = native.Context(max_n=1050, max_d=89, max_q=130)
    yield c
    c.close()


@pytest.fixture(scope="module")
def late_state():
    data = np.load(GOLDEN)
    n = int(data["ns"][-1])
    X, f = data["X"][:n], data["f"][:n]
    res = O.weighted_pca(X, f, False, 0.95, 0, noise=np.random.default_rng(n).normal(0.0, 1e-8, size=X.shape))
    return np.ascontiguousarray(res.Z), np.asarray(f, dtype=np.float64)


def test_posterior_matches_the_reference(native, ctx, late_state, capsys):
    rows = []
    for n, k, q, kernel, noise, user in CASES:
        Z, y = ard_state(500 + n + k, n, k)
        nb = np.vstack([Z.min(0) - 0.25, Z.max(0) + 0.5]) if user else None
        Xq = _queries(Z, q, n + q)
        ctx.gp_condition(y, Z=Z, norm_bounds=nb, kernel=KERNEL[kernel])
        out = ctx.gp_posterior(Xq, observation_noise=noise, covariance=True)
        ref = posterior(O.ExactGP(Z, y, nb, kernel=kernel), Xq, noise)
        assert out["mean"].shape == (q,) and out["variance"].shape == (q,) and out["covariance"].shape == (q, q)
        rows.append(((n, k, q), _errors(out, ref)))
    Z, y = late_state
    Xq = _queries(Z, 130, 1)
    ctx.gp_condition(y, Z=Z)
    rows.append(((Z.shape[0], Z.shape[1], 130), _errors(ctx.gp_posterior(Xq, covariance=True), posterior(O.ExactGP(Z, y), Xq))))
    with capsys.disabled():
        print("\n  gp_posterior vs reference, (n, k, q): mean, variance, covariance")
        for shape, e in rows:
            print(f"  {shape}: {e[0]:.2e} {e[1]:.2e} {e[2]:.2e}")
        print("  worst: " + " ".join(f"{max(e[i] for _, e in rows):.2e}" for i in range(3))
              + f" (tolerances {TOL_MEAN:.1e} {TOL_VAR:.1e} {TOL_COV:.1e})")
    for shape, (em, ev, ec) in rows:
        assert em <= TOL_MEAN and ev <= TOL_VAR and ec <= TOL_COV, (shape, em, ev, ec)


def test_bit_identities_with_the_scoring_path(native, ctx):
    for n, k, q in ((130, 9, 65), (449, 41, 130)):
        Z, y = ard_state(500 + n + k, n, k)
        Xq = _queries(Z, q, 3)
        ctx.gp_condition(y, Z=Z)
        a = ctx.gp_posterior(Xq, covariance=True)
        ucb0 = ctx.acq_eval(Xq, best_f=0.0, maximize=True, acq=native.ACQ_UCB, grad=False)      # kappa = 0: fma(0, sigma, mean)
        assert a["mean"].tobytes() == ucb0.tobytes(), (n, k, q)
        b = ctx.gp_posterior(Xq, covariance=True)
        plain = ctx.gp_posterior(Xq)
        for key in ("mean", "variance"):
            assert a[key].tobytes() == b[key].tobytes() == plain[key].tobytes(), key
        cov = a["covariance"]
        assert cov.tobytes() == b["covariance"].tobytes()
        assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes()
        free = a["variance"] > 1e-10
        assert free.sum() >= q - 1 and np.array_equal(np.diag(cov)[free], a["variance"][free])
        noisy = ctx.gp_posterior(Xq, observation_noise=True, covariance=True)
        assert np.array_equal(np.diag(noisy["covariance"]), noisy["variance"])       # the floor cannot act: s2 s_y^2 is above it
        assert noisy["mean"].tobytes() == a["mean"].tobytes()
        off = ~np.eye(q, dtype=bool)
        assert np.array_equal(noisy["covariance"][off], cov[off])
        sy = ctx.gp_state()["y_std"]
        want = ((a["variance"][free] / (sy * sy)) + 0.006737946999085467) * (sy * sy)
        assert (np.abs(noisy["variance"][free] - want) <= 4 * np.spacing(want)).all()


def test_the_floor(native, ctx):
    Z, y = ard_state(7, 65, 5)
    y = (y - y.mean()) / y.std(ddof=1) * 1e-6                   # s_y = 1e-6: above Standardize's 1e-8 guard, every variance <= 1e-12
    Xq = _queries(Z, 65, 4)
    ctx.gp_condition(y, Z=Z)
    out = ctx.gp_posterior(Xq, covariance=True)
    assert (out["variance"] == 1e-10).all()
    d = np.diag(out["covariance"])
    assert (d > 0.0).all() and (d < 1e-10).all()
    ref = posterior(O.ExactGP(Z, y), Xq)
    assert abs(ref["y_std"] - 1e-6) < 1e-12
    _assert_close(out, ref, "floor")


def test_fitted_models(native, ctx, capsys):
    Z, y = ard_state(2, 65, 5)
    Xq = _queries(Z, 65, 5)
    hp = ctx.gp_fit(y, Z=Z)
    assert hp["mean_constant"] != 0.0
    es = _assert_close(ctx.gp_posterior(Xq, observation_noise=True, covariance=True),
                       posterior(fitted_gp(Z, y, scalar_fit_as_ard(hp, 5)), Xq, True), "gp_fit")
    hp = ctx.gp_fit_ard(y, Z=Z)
    ea = _assert_close(ctx.gp_posterior(Xq, observation_noise=True, covariance=True),
                       posterior(fitted_gp(Z, y, hp), Xq, True), "gp_fit_ard")
    with capsys.disabled():
        print("\n  fitted states (65, 5, 65), mean / variance / covariance: scalar fit " + " ".join(f"{v:.2e}" for v in es)
              + "; ARD fit " + " ".join(f"{v:.2e}" for v in ea))


# ---- a batch: every run bit for bit what it takes alone ---------------------------------------------------------------------
B, N, D, Q = 4, 130, 12, 65
LO = (1.0, 0.5, 0.2, 0.05)


def _batch_state(b):
    rng = np.random.default_rng(21 + b)
    X = rng.uniform(-5, 5, (N, D)) * np.linspace(1, LO[b], D)
    y = np.sin(0.7 * X[:, 0]) * 40 + (X ** 2).sum(1) + rng.normal(size=N)
    return X, y, rng.normal(0, 1e-8, X.shape)


def _same(a, b):
    return a is not None and all(a[key].tobytes() == b[key].tobytes() for key in ("mean", "variance", "covariance"))


@pytest.fixture(scope="module")
def batch_data():
    X, y, noise = (np.stack(a) for a in zip(*[_batch_state(b) for b in range(B)]))
    return X, y, noise, np.argsort(np.argsort(y, axis=1), axis=1).astype(np.int64) + 1


def _batch_and_singles(native, batch_data):
    """A fresh batch with its conditioning in flight, one fresh context per run holding the run's own weighted PCA, the runs' k and
    Q queries per run inside its search box."""
    X, y, noise, ranks = batch_data
    bt = native.Batch(B, max_n=N, max_d=D, max_q=Q)
    bt.wpca_gp_condition_begin(X, ranks, noise, y)
    ks = [r["k"] for r in bt.wpca_results()]
    assert len(set(ks)) >= 2, ks                                # the runs differ in k (k_dev is read per run)
    singles = []
    for b in range(B):
        singles.append(native.Context(max_n=N, max_d=D, max_q=Q))
        assert singles[b].wpca(X[b], ranks=ranks[b], noise=noise[b])["k"] == ks[b]
    boxes = bt.acq_bounds()
    Xq = [np.random.default_rng(40 + b).uniform(boxes[b][0], boxes[b][1], size=(Q, ks[b])) for b in range(B)]
    return bt, singles, ks, Xq


def test_batch_equals_alone(native, batch_data):
    y = batch_data[1]
    bt, singles, ks, Xq = _batch_and_singles(native, batch_data)
    try:
        with pytest.raises(native.PcaboError) as e:             # the conditioning has not been waited for
            bt.gp_posterior(Xq)
        assert e.value.code == -1
        _, status = bt.gp_wait_eval(Xq, y.min(axis=1))
        assert (status == 0).all()
        out = bt.gp_posterior(Xq, covariance=True)
        for b, c in enumerate(singles):
            c.gp_condition(y[b])
            assert _same(out[b], c.gp_posterior(Xq[b], covariance=True)), b
    finally:
        for c in singles:
            c.close()
        bt.close()


def test_batch_equals_alone_after_the_lock_step_fit(native, batch_data):
    y = batch_data[1]
    bt, singles, ks, Xq = _batch_and_singles(native, batch_data)
    try:
        fits = bt.gp_fit()
        assert len({f["noise"] for f in fits}) == B              # every run reads its own lengthscale and noise
        for b, c in enumerate(singles):
            assert c.gp_fit(y[b])["theta"].tobytes() == fits[b]["theta"].tobytes()
        for noisy in (False, True):
            out = bt.gp_posterior(Xq, observation_noise=noisy, covariance=True)
            for b, c in enumerate(singles):
                assert _same(out[b], c.gp_posterior(Xq[b], observation_noise=noisy, covariance=True)), (b, noisy)
        bt.set_active([1, 0, 1, 1])
        parked = bt.gp_posterior(Xq)                             # a parked run is skipped, the others are served as before
        assert parked[1] is None and all(parked[b]["mean"].tobytes() == out[b]["mean"].tobytes() for b in (0, 2, 3))
    finally:
        for c in singles:
            c.close()
        bt.close()


def test_refusals_leave_the_context_usable(native):
    Z, y = ard_state(11, 40, 3)
    Xq = _queries(Z, 16, 6)
    xq = np.ascontiguousarray(Xq)
    c = native.Context(max_n=64, max_d=3, max_q=32)
    lib, h = native.LIB, None
    try:
        c.k = 3
        mean = np.empty(16)

        def refused(call):
            with pytest.raises(native.PcaboError) as e:
                call()
            assert e.value.code == -1

        refused(lambda: c.gp_posterior(Xq))                                                   # never conditioned
        c.gp_condition(y, Z=Z)
        good = c.gp_posterior(Xq, covariance=True)
        h = c._h
        for call in (lambda: c.gp_posterior(Xq[:0]),                                          # q < 1
                     lambda: c.gp_posterior(np.zeros((33, 3))),                               # q > max_q
                     lambda: c._chk(lib.pcabo_gp_posterior(h, xq.ctypes.data, 16, 0, None, None, None)),          # no output
                     lambda: c._chk(lib.pcabo_gp_posterior(h, xq.ctypes.data, 16, 2, mean.ctypes.data, None, None))):  # flag bits
            refused(call)
            again = c.gp_posterior(Xq, covariance=True)
            assert all(again[key].tobytes() == good[key].tobytes() for key in good)
        c.gp_condition(y, Z=Z, wait=False)
        refused(lambda: c.gp_posterior(Xq))                                                   # between _begin and _end
        c.gp_wait()
        assert c.gp_posterior(Xq)["mean"].tobytes() == good["mean"].tobytes()
        Zc = Z.copy()
        Zc[:, 1] = 0.5                                                                        # a Normalize range of 0: K is not finite
        with pytest.raises(native.PcaboError):
            c.gp_condition(y, Z=Zc)
        refused(lambda: c.gp_posterior(Xq))                                                   # the last conditioning left no GP
        c.gp_condition(y, Z=Z)
        again = c.gp_posterior(Xq, covariance=True)
        assert all(again[key].tobytes() == good[key].tobytes() for key in good)
    finally:
        c.close()


def test_device_pointer_mode_equals_host_pointer_mode(native):
    Z, y = ard_state(12, 70, 4)
    Xq = np.ascontiguousarray(_queries(Z, 65, 8))
    c = native.Context(max_n=70, max_d=4, max_q=65)
    try:
        c.gp_condition(y, Z=Z)
        host = c.gp_posterior(Xq, observation_noise=True, covariance=True)
        dev = torch.device("cuda:0")
        tX = torch.from_numpy(Xq).to(dev)
        tm, tv, tc = (torch.zeros(s, dtype=torch.float64, device=dev) for s in (65, 65, 65 * 65))
        torch.cuda.synchronize()             # the context's stream is not ordered with torch's: hand over finished tensors
        assert native.LIB.pcabo_set_pointer_mode(c._h, native.PTR_DEVICE) == 0
        c._chk(native.LIB.pcabo_gp_posterior(c._h, tX.data_ptr(), 65, native.POST_OBS_NOISE, tm.data_ptr(), tv.data_ptr(), tc.data_ptr()))
        assert native.LIB.pcabo_set_pointer_mode(c._h, native.PTR_HOST) == 0
        for key, t in (("mean", tm), ("variance", tv), ("covariance", tc)):
            assert t.cpu().numpy().tobytes() == host[key].tobytes(), key
    finally:
        c.close()


# ---- the optimiser classes: a query between two iterations changes nothing -----------------------------------------------------
def _probing(base):
    class Probing(base):
        def optimize_acqf_and_get_observation(self):
            new = super().optimize_acqf_and_get_observation()
            self.seen = (np.array(self.x_evals), np.array(self.f_evals, dtype=np.float64),
                         self.posterior(self.probe, covariance=True))
            return new
    return Probing


@pytest.mark.parametrize("acq_kernel", ["latency", "group"])
def test_pca_bo_trajectory_is_unchanged_by_posterior_calls(acq_kernel):
    from Algorithms import PCA_BO
    runs = []
    for cls in (PCA_BO, _probing(PCA_BO)):
        opt = cls(budget=45, n_DoE=30, random_seed=15101, acq_kernel=acq_kernel)
        opt.probe = np.random.default_rng(3).uniform(-5.0, 5.0, size=(70, 10))
        opt(problem=BBOBProblem(15, 0, 10), dim=10, bounds=np.array([-5.0, 5.0]))
        runs.append(opt)
    plain, probed = runs
    assert np.array(plain.x_evals).tobytes() == np.array(probed.x_evals).tobytes()
    assert np.array(plain.f_evals, dtype=np.float64).tobytes() == np.array(probed.f_evals, dtype=np.float64).tobytes()
    post = probed.seen[2]
    assert post["covariance"].shape == (70, 70) and np.isfinite(post["covariance"]).all() and (post["variance"] >= 1e-10).all()
    with pytest.raises(RuntimeError):
        probed.posterior(probed.probe)                                                        # the run is over


def test_vanilla_bo_posterior_matches_the_reference():
    from Algorithms import Vanilla_BO
    opt = _probing(Vanilla_BO)(budget=14, n_DoE=10, random_seed=15051)
    opt.probe = np.random.default_rng(4).uniform(-5.0, 5.0, size=(20, 4))
    opt(problem=BBOBProblem(15, 0, 4), dim=4, bounds=np.array([-5.0, 5.0]))
    X, f, out = opt.seen
    assert X.shape == (13, 4)
    gp = O.ExactGP(X, f, np.vstack([np.zeros(4), np.ones(4)]))
    _assert_close(out, posterior(gp, opt.probe), "Vanilla_BO")
