"""GP posterior samples on the MI355X (pcabo_gp_posterior_sample / pcabo_batch_gp_posterior_sample: launch_posterior,
k_post_chol_prep, launch_cholesky, k_post_sample; Context.gp_posterior_samples, Batch.gp_posterior_samples, PCA_BO.posterior_samples,
Vanilla_BO.posterior_samples).

Shapes (n, k, q, S): posterior_samples_reference.SHAPES - one block with 63 identity rows (q = 1), a partial tile (63), an exact tile
(64, S = 64), a second block that is almost all padding with S across a tile (65, 65), three blocks with a tile strictly below the
diagonal and partial last tiles in q and S (130, 130).

Bounds.  Factor (backward, derived): max |Lc Lc^T - A|_ab / sqrt(A_aa A_bb) <= 8 (q + 1) 2^-53, Higham's gamma_{q+1} |L| |L^T| for any
summation order with |L||L^T|_ab <= sqrt(A_aa A_bb) and a factor 8 for the square roots and divisions; it does not depend on the
conditioning.  Product (derived): |samples - (mean + base Lc^T)|_sa <= 4 (q + 2) 2^-53 (|mean_a| + sum_b |base_sb| |Lc_ab|), gamma_{q+1}
of a q-term inner product plus the mean's addition, with a factor 4 of head room for the constants; the right sides are formed in long
double from the device's own Lc and mean.  Forward (measured): |d| / (s_y max(1, |base_s|_2)) against the long-double reference on the
well-conditioned inputs of tests/test_posterior_samples_cpu.py, asserted at 10 x the largest value measured on an MI355X:
MEASURED_FWD below, per shape in EXPERIMENTS.md "GP posterior samples".
"""
import numpy as np
import pytest
import torch

import pcabo_oracle as O
from ard_reference import ard_state
from pcabo.bbob import BBOBProblem
from posterior_samples_reference import (KERNEL, RUNGS, SHAPES, base_samples, nasty_queries, plain_queries, posterior_samples,
                                         state)

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
# forward errors measured on an MI355X per row of SHAPES (plain queries, observation noise on); the assertion is 10 x the largest
MEASURED_FWD = (1.41e-14, 3.76e-14, 3.71e-14, 3.43e-15, 9.62e-15)
TOL_FWD = 10.0 * max(MEASURED_FWD)


@pytest.fixture(scope="module")
def ctx(native):
    torch.set_num_threads(8)
    c = native.Context(max_n=257, max_d=9, max_q=192)
    yield c
    c.close()


def _condition(ctx, shape):
    Z, y, nb = state(shape)
    ctx.gp_condition(y, Z=Z, norm_bounds=nb, kernel=KERNEL[shape[4]])
    return Z, y, nb


def _factor(ctx, Xq, noise):
    """The device's Lc read exactly (centred, base = I), its rung and A = cov + rung s_y^2 I in long double."""
    q = Xq.shape[0]
    out = ctx.gp_posterior_samples(Xq, base_samples=np.eye(q), observation_noise=noise, centred=True)
    assert out["samples"].shape == (q, q) and out["jitter"] in RUNGS
    Lc = np.ascontiguousarray(out["samples"].T)
    post = ctx.gp_posterior(Xq, observation_noise=noise, covariance=True)
    sy = LD(ctx.gp_state()["y_std"])
    A = post["covariance"].astype(LD) + LD(out["jitter"]) * sy * sy * np.eye(q, dtype=LD)
    return Lc, out, post, A


def _backward_error(Lc, A):
    L = Lc.astype(LD)
    d = np.sqrt(np.diag(A))
    return float((np.abs(L @ L.T - A) / np.outer(d, d)).max())


def test_factor_backward_error_within_the_derived_bound(native, ctx, capsys):
    rows = []
    for shape in SHAPES:
        n, k, q, S, kernel, noise, user = shape
        Z, y, nb = _condition(ctx, shape)
        for what, Xq in (("plain", plain_queries(Z, q, n + q)), ("nasty", nasty_queries(Z, q, n + q))):
            Lc, out, post, A = _factor(ctx, Xq, noise)
            assert np.isfinite(Lc).all() and (np.triu(Lc, 1) == 0.0).all(), (shape, what)         # exactly zero above the diagonal
            assert (np.diag(Lc) > 0.0).all(), (shape, what)
            rows.append((shape[:4], what, out["jitter"], _backward_error(Lc, A), 8 * (q + 1) * U))
    with capsys.disabled():
        print("\n  Lc Lc^T against A, (n, k, q, S) queries: rung, error, bound")
        for r in rows:
            print(f"  {r[0]} {r[1]}: {r[2]:g} {r[3]:.2e} {r[4]:.2e}")
    for shape, what, jitter, err, bound in rows:
        assert err <= bound, (shape, what, jitter, err, bound)


def test_product_within_the_derived_bound(native, ctx, capsys):
    rows = []
    for shape in SHAPES:
        n, k, q, S, kernel, noise, user = shape
        Z, y, nb = _condition(ctx, shape)
        Xq = nasty_queries(Z, q, n + q)
        Lc, _, post, _ = _factor(ctx, Xq, noise)
        base = base_samples(q, S)
        out = ctx.gp_posterior_samples(Xq, base_samples=base, observation_noise=noise)
        cen = ctx.gp_posterior_samples(Xq, base_samples=base, observation_noise=noise, centred=True)
        assert out["samples"].shape == (S, q) and out["mean"].shape == (q,)
        assert out["mean"].tobytes() == cen["mean"].tobytes() == post["mean"].tobytes()
        Lx, bx, mean = Lc.astype(LD), base.astype(LD), post["mean"].astype(LD)
        prod, mag = bx @ Lx.T, np.abs(bx) @ np.abs(Lx).T
        worst = 0.0
        for got, m in ((out["samples"], mean), (cen["samples"], np.zeros(q, dtype=LD))):
            err = np.abs(got.astype(LD) - (m + prod))
            bound = 4 * (q + 2) * U * (np.abs(m) + mag)
            assert (err <= bound).all(), (shape, float((err / np.maximum(bound, LD(1e-300))).max()))
            worst = max(worst, float((err / np.maximum(bound, LD(1e-300))).max()))
        rows.append((shape[:4], worst))
    with capsys.disabled():
        print("\n  samples against mean + base Lc^T, (n, k, q, S): worst error / bound")
        for r in rows:
            print(f"  {r[0]}: {r[1]:.3f}")


def test_forward_error_against_the_reference(native, ctx, capsys):
    """Measured on an MI355X, in the order of SHAPES: 1.41e-14, 3.76e-14, 3.71e-14, 3.43e-15, 9.62e-15 (cond_2(A) 1.0, 81, 52, 13, 17);
    the Vanilla_BO run below 1.65e-16.  Asserted: 10 x the largest, 3.76e-13."""
    rows = []
    for shape in SHAPES:
        n, k, q, S, kernel = shape[:5]
        Z, y, nb = _condition(ctx, shape)
        Xq = plain_queries(Z, q, n + q)
        base = base_samples(q, S)
        out = ctx.gp_posterior_samples(Xq, base_samples=base, observation_noise=True)
        ref = posterior_samples(O.ExactGP(Z, y, nb, kernel=kernel), Xq, base, observation_noise=True)
        assert out["jitter"] == ref["jitter"] == 0.0 and ref["cond"] <= 1e6
        unit = ref["y_std"] * np.maximum(1.0, np.linalg.norm(base, axis=1))[:, None]
        rows.append((shape[:4], float((np.abs(out["samples"].astype(LD) - ref["samples"]) / unit).max()), ref["cond"]))
    with capsys.disabled():
        print("\n  samples against the long-double reference, (n, k, q, S): |d| / (s_y max(1, |base_s|)), cond_2(A)")
        for r in rows:
            print(f"  {r[0]}: {r[1]:.2e} {r[2]:.1e}")
        print(f"  worst {max(r[1] for r in rows):.2e} (tolerance {TOL_FWD:.1e})")
    for shape, err, _ in rows:
        assert err <= TOL_FWD, (shape, err)


def test_two_calls_give_the_same_bytes_and_later_calls_are_unchanged(native, ctx):
    shape = SHAPES[4]
    n, k, q, S = shape[:4]
    Z, y, nb = _condition(ctx, shape)
    Xq = nasty_queries(Z, q, 5)
    box = ctx.acq_bounds()
    ics = np.random.default_rng(9).uniform(box[0], box[1], size=(10, k))
    best = float(y.min())

    def later():
        post = ctx.gp_posterior(Xq, observation_noise=True, covariance=True)
        val, grad = ctx.acq_eval(Xq[:32], best_f=best, maximize=False, acq=native.ACQ_LOG_EI, grad=True)
        cand, vals = ctx.optimize_acqf(ics, box, best)[:2]
        return [post["mean"], post["variance"], post["covariance"], val, grad, cand, vals]

    before = later()
    a = ctx.gp_posterior_samples(Xq, n_samples=S, seed=3)
    b = ctx.gp_posterior_samples(Xq, n_samples=S, seed=3)
    assert all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in ("samples", "mean", "jitter"))
    assert a["samples"].tobytes() != ctx.gp_posterior_samples(Xq, n_samples=S, seed=4)["samples"].tobytes()
    after = later()
    assert all(x.tobytes() == z.tobytes() for x, z in zip(before, after))


# ---- a batch: every run bit for bit what it takes alone ---------------------------------------------------------------------
B, N, D, Q, S_B = 3, 130, 9, 130, 65
LO = (1.0, 0.3, 0.05)


def _batch_state(b):
    rng = np.random.default_rng(21 + b)
    X = rng.uniform(-5, 5, (N, D)) * np.linspace(1, LO[b], D)
    y = np.sin(0.7 * X[:, 0]) * 40 + (X ** 2).sum(1) + rng.normal(size=N)
    return X, y, rng.normal(0, 1e-8, X.shape)


def _same(a, b):
    return a is not None and all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in ("samples", "mean", "jitter"))


@pytest.mark.parametrize("fitted", [False, True])
def test_batch_equals_alone(native, fitted):
    """A fresh batch per state, as tests/test_gpu_posterior.py does; fitted: after pcabo_batch_gp_fit every run samples from its own
    fitted model."""
    X, y, noise = (np.stack(a) for a in zip(*[_batch_state(b) for b in range(B)]))
    ranks = np.argsort(np.argsort(y, axis=1), axis=1).astype(np.int64) + 1
    bt = native.Batch(B, max_n=N, max_d=D, max_q=Q)
    singles = []
    try:
        bt.wpca_gp_condition_begin(X, ranks, noise, y)
        ks = [r["k"] for r in bt.wpca_results()]
        assert len(set(ks)) >= 2, ks                            # the runs differ in k
        for b in range(B):
            singles.append(native.Context(max_n=N, max_d=D, max_q=Q))
            assert singles[b].wpca(X[b], ranks=ranks[b], noise=noise[b])["k"] == ks[b]
        boxes = bt.acq_bounds()
        Xq = [np.random.default_rng(40 + b).uniform(boxes[b][0], boxes[b][1], size=(Q, ks[b])) for b in range(B)]
        base = np.stack([np.random.default_rng(60 + b).standard_normal((S_B, Q)) for b in range(B)])
        if fitted:
            fits = bt.gp_fit()
            assert len({f["noise"] for f in fits}) == B         # every run reads its own lengthscale and noise
            for b, c in enumerate(singles):
                assert c.gp_fit(y[b])["theta"].tobytes() == fits[b]["theta"].tobytes()
        else:
            with pytest.raises(native.PcaboError) as e:         # the conditioning has not been waited for
                bt.gp_posterior_samples(Xq, base_samples=base)
            assert e.value.code == -1
            _, status = bt.gp_wait_eval(Xq, y.min(axis=1))
            assert (status == 0).all()
            for b, c in enumerate(singles):
                c.gp_condition(y[b])
        bt.set_active([1, 0, 1])
        for noisy, centred in ((False, False), (True, True)):
            out = bt.gp_posterior_samples(Xq, base_samples=base, observation_noise=noisy, centred=centred)
            assert out[1] is None and list(bt.sample_status) == [0, -1, 0]
            for b in (0, 2):
                alone = singles[b].gp_posterior_samples(Xq[b], base_samples=base[b], observation_noise=noisy, centred=centred)
                assert _same(out[b], alone), (noisy, b)
        # the parked run's output blocks are left as they are
        buf = np.zeros((B, Q * D))
        for b in range(B):
            buf[b, : Xq[b].size] = Xq[b].ravel()
        samples, mean, jit = np.full((B, S_B, Q), 7.0), np.full((B, Q), 7.0), np.full(B, 7.0)
        status = np.zeros(B, dtype=np.int32)
        bt._chk(native.LIB.pcabo_batch_gp_posterior_sample(bt._h, buf.ctypes.data, Q, 0, base.ctypes.data, S_B, samples.ctypes.data,
                                                           mean.ctypes.data, jit.ctypes.data, status.ctypes.data))
        assert list(status) == [0, -1, 0]
        assert (samples[1] == 7.0).all() and (mean[1] == 7.0).all() and jit[1] == 7.0
        assert samples[0].tobytes() == singles[0].gp_posterior_samples(Xq[0], base_samples=base[0])["samples"].tobytes()
    finally:
        for c in singles:
            c.close()
        bt.close()


def test_refusals_leave_the_context_usable(native):
    Z, y = ard_state(11, 40, 3)
    Xq = np.ascontiguousarray(plain_queries(Z, 16, 6))
    c = native.Context(max_n=64, max_d=3, max_q=32)
    lib = native.LIB
    try:
        c.k = 3
        base = np.random.default_rng(1).standard_normal((1025, 16))
        big = np.zeros((1025, 33))
        out, mean = np.zeros((1025, 33)), np.empty(33)

        def raw(xq=Xq, q=16, flags=0, b=base, S=8, o=out):
            return lib.pcabo_gp_posterior_sample(c._h, xq.ctypes.data, q, flags, None if b is None else b.ctypes.data, S,
                                                 None if o is None else o.ctypes.data, mean.ctypes.data, None)

        assert raw() == -1                                                                    # never conditioned
        c.gp_condition(y, Z=Z)
        good = c.gp_posterior_samples(Xq, base_samples=base[:8])
        post = c.gp_posterior(Xq, covariance=True)
        for call in (lambda: raw(S=0), lambda: raw(S=1025), lambda: raw(xq=big, q=33, b=big), lambda: raw(b=None),
                     lambda: raw(o=None), lambda: raw(flags=4), lambda: raw(flags=7)):
            assert call() == -1
            assert (out == 0.0).all()                                                         # nothing was written
            again = c.gp_posterior_samples(Xq, base_samples=base[:8])
            assert again["samples"].tobytes() == good["samples"].tobytes() and again["jitter"] == good["jitter"]
        assert raw(S=1024) == 0 and raw(flags=3) == 0                                         # the largest S, both flags
        with pytest.raises(native.PcaboError) as e:                                           # gp_posterior still refuses flag 2
            c._chk(lib.pcabo_gp_posterior(c._h, Xq.ctypes.data, 16, 2, mean.ctypes.data, None, None))
        assert e.value.code == -1
        c.gp_condition(y, Z=Z, wait=False)
        assert raw() == -1                                                                    # between _begin and _end
        c.gp_wait()
        assert c.gp_posterior_samples(Xq, base_samples=base[:8])["samples"].tobytes() == good["samples"].tobytes()
        again = c.gp_posterior(Xq, covariance=True)
        assert all(again[key].tobytes() == post[key].tobytes() for key in post)
    finally:
        c.close()


# ---- the optimiser classes: sampling between two iterations changes nothing -----------------------------------------------------
def _probing(base, **kw):
    class Probing(base):
        def optimize_acqf_and_get_observation(self):
            new = super().optimize_acqf_and_get_observation()
            self.seen = (np.array(self.x_evals), np.array(self.f_evals, dtype=np.float64))
            self.draws = self.posterior_samples(self.probe, n_samples=4, seed=len(self.f_evals), **kw)
            return new
    return Probing


@pytest.mark.parametrize("acq_kernel", ["latency", "group"])
def test_pca_bo_trajectory_is_unchanged_by_sampling_calls(acq_kernel):
    from Algorithms import PCA_BO
    runs = []
    for cls in (PCA_BO, _probing(PCA_BO)):
        opt = cls(budget=40, n_DoE=20, random_seed=15101, acq_kernel=acq_kernel)
        opt.probe = np.random.default_rng(3).uniform(-5.0, 5.0, size=(70, 10))
        opt(problem=BBOBProblem(15, 0, 10), dim=10, bounds=np.array([-5.0, 5.0]))
        runs.append(opt)
    plain, probed = runs
    assert np.array(plain.x_evals).tobytes() == np.array(probed.x_evals).tobytes()
    assert np.array(plain.f_evals, dtype=np.float64).tobytes() == np.array(probed.f_evals, dtype=np.float64).tobytes()
    draws = probed.draws
    assert draws["samples"].shape == (4, 70) and np.isfinite(draws["samples"]).all() and draws["jitter"] in RUNGS
    with pytest.raises(RuntimeError):
        probed.posterior_samples(probed.probe)                                                # the run is over


def test_vanilla_bo_samples_match_the_reference():
    """Observation noise on: cond_2(A) <= q (1 + s2) / s2 = 20 * 149.4 < 1e6 whatever the points, the forward test's condition."""
    from Algorithms import Vanilla_BO
    opt = _probing(Vanilla_BO, observation_noise=True)(budget=14, n_DoE=10, random_seed=15051)
    opt.probe = np.random.default_rng(4).uniform(-5.0, 5.0, size=(20, 4))
    opt(problem=BBOBProblem(15, 0, 4), dim=4, bounds=np.array([-5.0, 5.0]))
    X, f = opt.seen
    assert X.shape == (13, 4)
    base = np.random.default_rng(13).standard_normal((4, 20))
    ref = posterior_samples(O.ExactGP(X, f, np.vstack([np.zeros(4), np.ones(4)])), opt.probe, base, observation_noise=True)
    assert opt.draws["jitter"] == ref["jitter"] == 0.0 and ref["cond"] <= 1e6
    unit = ref["y_std"] * np.maximum(1.0, np.linalg.norm(base, axis=1))[:, None]
    err = float((np.abs(opt.draws["samples"].astype(LD) - ref["samples"]) / unit).max())
    print(f"  Vanilla_BO (13, 4, 20, 4): {err:.2e} (tolerance {TOL_FWD:.1e})")
    assert err <= TOL_FWD, err
