"""GP posterior queries on the device against an extended-precision reference at edge shapes.

`pcabo_gp_posterior` / `pcabo_batch_gp_posterior` (`k_score_ks`, `k_score_gemm` with the V store, `k_post_combine`,
`k_post_cov`: kernels_post.hip) are judged in the error units of `acq_reference.posterior` (first-order analysis of
any fp64 implementation; `test_ucb_posterior_reference_cpu.py` shows a numpy restatement staying under 4 of each and
wrong variants leaving them): the mean, the floored variance - exactly 1e-10 where the reference's raw variance is
below the floor - and EVERY entry of the covariance in its own unit, so that the cancellation k(a, b) - v_a . v_b is
held at the precision where it matters: a duplicated query, two pairs 1e-9 apart (one inside a 64 x 64 tile, one
across two), queries on training points.  The limit is 16 units, as in the other edge tests; `test_gpu_posterior.py`
compares with a float64 oracle at tolerances measured on the device.

The reference starts from each object's OWN conditioned state (`gp_state()`), read once and taken as exact.

Beside the small states, n257 and n513, the four stress states of `acq_reference.STATES`: n385k65 and n449k83 - the
second `c0 += 64` trip of `k_post_cov` (k > 64) over 7 and 8 panels of V; n1025 - `k_post_cov` over 17 panels,
five `k_score_ks` blocks, 17 row blocks of `k_score_gemm` and as many records per query for `k_post_combine`; n1473 -
24 panels, six blocks, 24 row blocks and records (more than 18).
"""
import time

import numpy as np
import pytest

import acq_reference as A

pytestmark = pytest.mark.gpu

LIMIT = 16.0
PATHS = ("context", "batch")


@pytest.mark.parametrize("name", A.POSTERIOR_STATES)
def test_posterior_against_the_reference(native, name, capsys):
    """Per state, on `Context.gp_posterior` and `Batch(1).gp_posterior`, at the query prefixes 1, 15, 16, 17 (the
    16-query blocks of `k_score_ks`), 63, 64, 65 (a partial, an exact, an exact-plus-one covariance tile) and 130
    (three tile rows, off-diagonal tiles, a partial last one), with and without the observation noise: mean, floored
    variance and every covariance entry within 16 units; cov == cov^T and mean / variance with and without the
    covariance bit for bit.  Prints the worst ratios per path."""
    t0 = time.time()
    st, _, _ = A.prepared(name)
    n, k, Z, y, X = st.n, st.k, st.Z, st.y, st.X
    kcode = native.KERNEL_RBF if st.kernel == "rbf" else native.KERNEL_MATERN52
    ctx = native.Context(max_n=n, max_d=k, max_q=A.Q)
    bt = native.Batch(1, max_n=n, max_d=k, max_q=A.Q)
    worst, fails = {}, []
    try:
        ctx.gp_condition(y, Z=Z, norm_bounds=st.norm_bounds, lengthscale=st.lengthscale, noise=st.noise, kernel=kcode)
        bt.gp_condition_begin(Z[None], y[None], norm_bounds=st.norm_bounds, lengthscale=st.lengthscale, gp_noise=st.noise,
                              kernel=kcode)
        _, status = bt.gp_wait_eval([X], [float(y.min())])
        assert not status.any()
        for path, owner, query in (("context", ctx, lambda Xq, **kw: ctx.gp_posterior(Xq, **kw)),
                                   ("batch", bt.ctx[0], lambda Xq, **kw: bt.gp_posterior([Xq], **kw)[0])):
            state = owner.gp_state()
            if st.norm_bounds is not None:
                assert np.array_equal(state["norm_bounds"], st.norm_bounds)
            key, lin = A.cached_linear(st, state)
            assert A.check_posterior_conditions(name, st, lin) == [], (name, path)   # the device's own state, not skipped
            w = worst.setdefault(path, {"mean": 0.0, "variance": 0.0, "covariance": 0.0})
            for noise in (False, True):
                ref = A.cached_posterior(st, key, noise)
                if name in ("E", "mixed") and not (ref.clamped.all() if name == "E" else ref.clamped.any() and not ref.clamped.all()):
                    fails.append((path, noise, "the floor does not act as the state's name says"))
                for q in A.POST_PREFIXES:
                    full = query(X[:q], observation_noise=noise, covariance=True)
                    plain = query(X[:q], observation_noise=noise, covariance=False)
                    assert full is not None and plain is not None and "covariance" not in plain
                    assert full["mean"].shape == (q,) and full["variance"].shape == (q,) and full["covariance"].shape == (q, q)
                    for what, r in A.judge_posterior(ref, full).items():
                        w[what] = max(w[what], r)
                        if not r <= LIMIT:
                            fails.append((path, noise, q, what, r))
                    for what in ("mean", "variance"):
                        if full[what].tobytes() != plain[what].tobytes():
                            fails.append((path, noise, q, what, "differs with and without the covariance"))
                    cov = full["covariance"]
                    if cov.tobytes() != np.ascontiguousarray(cov.T).tobytes():
                        fails.append((path, noise, q, "the covariance is not symmetric bit for bit"))
            if (st.name, A.digest(owner.gp_state())) != key:
                fails.append((path, "the queries changed the conditioned state"))
    finally:
        ctx.close()
        bt.close()
    with capsys.disabled():
        print("\n[posterior, device / reference units, state %s (n=%d k=%d %s)] " % (name, n, k, st.kernel)
              + "; ".join("%s mean %.2g variance %.2g covariance %.2g" % (p, w["mean"], w["variance"], w["covariance"])
                          for p, w in worst.items()) + "; %.1f s" % (time.time() - t0))
    assert not fails, (len(fails), fails[:12])
    assert set(worst) == set(PATHS)
