"""The call-order rules of include/pcabo.h as the Python binding meets them, at the smallest shapes: every entry point with a rule
is called once in each wrong state and once in the right one, and a refusal is held to its return code and to the full text of
pcabo_last_error / pcabo_batch_last_error.  Every refusal here is a host-side check that returns before anything is launched.  The
texts below were copied from csrc/pcabo_api.hip as it stood before the call state moved into csrc/model_state.h: they are the
record of what callers have seen, not a product of the code under test.

Then the single-context calls on the members of a batch: after a full lock-step iteration acq_eval, gp_state and gp_posterior on
bt.ctx[b] equal a stand-alone context's results bit for bit, at n = 3 and again after a second conditioning at n = 4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -1
IN_FLIGHT = "%s: a conditioning is in flight, call pcabo_gp_condition_end first"
NO_GP = "%s: call pcabo_gp_condition first"
B_BUSY = "%s: a conditioning or a _begin call of this batch has not been ended"


def refused(call, text, code=ERR_ARG):
    with pytest.raises(Exception) as e:
        call()
    assert type(e.value).__name__ == "PcaboError", repr(e.value)
    assert e.value.code == code and str(e.value) == "libpcabo error %d: %s" % (code, text), str(e.value)


def data(B, n, d=2, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-5, 5, (B, n, d))
    y = rng.normal(size=(B, n)) * 50 + 300
    return X, y, np.argsort(np.argsort(y, axis=1), axis=1) + 1


def test_context_refusals(native):
    X, y, ranks = data(1, 3)
    X, y, ranks = X[0], y[0], ranks[0]
    c = native.Context(max_n=8, max_d=2, max_q=16)
    c.n, c.d, c.k = 3, 2, 1                            # (the binding shapes its arrays by these mirrors; the library has seen nothing)
    xq, box = np.zeros((2, 1)), np.array([[0.0], [1.0]])
    # ---- a new context: nothing enqueued, no GP ----
    refused(lambda: c.gp_condition(y), "pcabo_gp_condition: Z == NULL needs a matching pcabo_wpca call first")
    refused(lambda: c.wpca_results(), "pcabo_wpca_results: no weighted PCA enqueued")
    refused(lambda: c.gp_wait(), "pcabo_gp_condition_end: no conditioning in flight")
    refused(lambda: c.gp_wait_eval(xq, 0.0), "pcabo_gp_condition_end_eval: no conditioning in flight")
    refused(lambda: c.acq_bounds(), "pcabo_acq_bounds: call pcabo_gp_condition first")
    refused(lambda: c.acq_eval(xq, 0.0), NO_GP % "pcabo_acq_eval")
    refused(lambda: c.optimize_acqf(xq, box, 0.0), NO_GP % "pcabo_optimize_acqf")
    refused(lambda: c.gp_fit(y), "pcabo_gp_fit: Z == NULL needs a matching pcabo_wpca call first")
    refused(lambda: c.gp_posterior(xq), "pcabo_gp_posterior: no conditioned GP, call pcabo_gp_condition first")
    refused(lambda: c.gp_loo(), "pcabo_gp_loo: no conditioned GP, call pcabo_gp_condition first")
    refused(lambda: c.gp_extend(xq[:1], [0.0]), "pcabo_gp_extend: no conditioned GP, call pcabo_gp_condition first")
    refused(lambda: c.gp_truncate(3), "pcabo_gp_truncate: no conditioned GP, call pcabo_gp_condition first")
    refused(lambda: c.inverse_map(np.zeros(1)), "pcabo_inverse_map: call pcabo_wpca first")
    # ---- a weighted PCA alone: conditioning on its projection needs its very n and k ----
    k = c.wpca(X, ranks=ranks)["k"]
    c.inverse_map(np.zeros(k))
    xq, box = np.full((2, k), 0.25), np.array([[0.0] * k, [1.0] * k])
    refused(lambda: c.gp_condition(np.append(y, 1.0)), "pcabo_gp_condition: Z == NULL needs a matching pcabo_wpca call first")
    c.n = 3
    refused(lambda: c.gp_fit(np.append(y, 1.0)), "pcabo_gp_fit: Z == NULL needs a matching pcabo_wpca call first")
    c.n = 3
    refused(lambda: c.acq_eval(xq, 0.0), NO_GP % "pcabo_acq_eval")
    c.gp_condition(y)                                  # the right state for it
    c.gp_posterior(xq), c.gp_loo(), c.acq_eval(xq, 0.0), c.acq_bounds()
    refused(lambda: c.gp_wait(), "pcabo_gp_condition_end: no conditioning in flight")
    # ---- a conditioning in flight ----
    c.wpca_gp_condition(X, y, ranks=ranks)
    refused(lambda: c.wpca(X, ranks=ranks), "pcabo_wpca: a conditioning is in flight, call pcabo_gp_condition_end first")
    refused(lambda: c.wpca_gp_condition(X, y, ranks=ranks), IN_FLIGHT % "pcabo_wpca_gp_condition_begin")
    refused(lambda: c.gp_fit(y), IN_FLIGHT % "pcabo_gp_fit")
    refused(lambda: c.gp_posterior(xq), IN_FLIGHT % "pcabo_gp_posterior")
    refused(lambda: c.gp_loo(), IN_FLIGHT % "pcabo_gp_loo")
    refused(lambda: c.gp_extend(xq[:1], [0.0]), IN_FLIGHT % "pcabo_gp_extend")
    refused(lambda: c.gp_truncate(3), IN_FLIGHT % "pcabo_gp_truncate")
    refused(lambda: c.acq_eval(xq, 0.0), NO_GP % "pcabo_acq_eval")
    refused(lambda: c.optimize_acqf(xq, box, 0.0), NO_GP % "pcabo_optimize_acqf")
    assert c.acq_bounds().shape == (2, k)              # allowed: the box is there before the factorisation ends
    assert c.gp_wait_eval(xq, float(y.min())).shape == (2,)
    # ---- conditioned: everything that asks the model goes ahead ----
    c.optimize_acqf(xq, c.acq_bounds(), float(y.min()))
    assert c.gp_extend(xq[:1], [float(y.mean())]) == 4 and c.gp_truncate(3) == 3
    refused(lambda: c.gp_truncate(2), "pcabo_gp_truncate: n0 must lie in n_base .. n")
    refused(lambda: c.gp_wait_eval(xq, 0.0), "pcabo_gp_condition_end_eval: no conditioning in flight")
    c.wpca_gp_condition(X, y, ranks=ranks)
    c.gp_wait()
    fit = c.gp_fit(y)                                  # Z == NULL: the projection of the wPCA above
    assert np.isfinite(fit["loss"])
    c.acq_eval(xq, float(y.min()))                     # the context is left conditioned at the fit
    c.wpca(X, ranks=ranks)                             # a wPCA alone takes the GP away
    refused(lambda: c.acq_eval(xq, 0.0), NO_GP % "pcabo_acq_eval")
    c.close()


def test_batch_refusals(native):
    B = 2
    X, y, ranks = data(B, 3)
    bt = native.Batch(B, max_n=8, max_d=2, max_q=16)
    bt.n, bt.d, bt.k = 3, 2, np.ones(B, dtype=np.int32)      # (the binding shapes its arrays by these mirrors)
    bt.ctx[0].k = 1
    xq = [np.zeros((2, 1))] * B
    box = [np.array([[0.0], [1.0]])] * B
    best = [0.0] * B
    # ---- a new batch ----
    refused(lambda: bt.wpca_results(), "pcabo_batch_wpca_results: nothing enqueued")
    refused(lambda: bt.acq_bounds(), "pcabo_batch_acq_bounds: no conditioning enqueued")
    refused(lambda: bt.gp_wait_eval(xq, best), "pcabo_batch_gp_condition_end_eval: no conditioning in flight")
    refused(lambda: bt.gp_eval_begin(xq, best), "pcabo_batch_gp_condition_end_eval: no conditioning in flight")
    refused(lambda: bt.gp_eval_end((np.zeros((B, 4)), 2, np.zeros(B), 0, 0)), "pcabo_batch_gp_condition_end_eval_end: no _begin before it")
    refused(lambda: bt.gp_posterior(xq), "pcabo_batch_gp_posterior: no conditioned GP")
    refused(lambda: bt.gp_loo(), "pcabo_batch_gp_loo: no conditioned GP")
    refused(lambda: bt.gp_fit(), "pcabo_batch_gp_fit: call pcabo_batch_wpca_gp_condition_begin or pcabo_batch_gp_condition_begin first")
    refused(lambda: bt.optimize_acqf(xq, box, best), "pcabo_batch_optimize_acqf: no conditioned GP")
    refused(lambda: bt.optimize_begin(xq, box, best), "pcabo_batch_optimize_acqf_begin: no conditioned GP")
    refused(lambda: bt.optimize_end((2, 5)), "pcabo_batch_optimize_acqf_end: no matching _begin before it")
    refused(lambda: bt.inverse_map([np.zeros(1)] * B), "pcabo_batch_inverse_map: no weighted PCA collected")
    refused(lambda: bt.inverse_map_end(), "pcabo_batch_inverse_map_end: no _begin before it")
    # ---- a conditioning in flight, its wPCA not collected yet ----
    bt.wpca_gp_condition_begin(X, ranks, None, y)
    refused(lambda: bt.wpca_gp_condition_begin(X, ranks, None, y), "pcabo_batch_wpca_gp_condition_begin: a conditioning is in flight")
    refused(lambda: bt.gp_condition_begin(X, y), "pcabo_batch_gp_condition_begin: a conditioning is in flight")
    refused(lambda: bt.inverse_map([np.zeros(1)] * B), "pcabo_batch_inverse_map: no weighted PCA collected")
    refused(lambda: bt.gp_posterior(xq), B_BUSY % "pcabo_batch_gp_posterior")
    refused(lambda: bt.gp_loo(), B_BUSY % "pcabo_batch_gp_loo")
    refused(lambda: bt.optimize_acqf(xq, box, best), "pcabo_batch_optimize_acqf: no conditioned GP")
    refused(lambda: bt.ctx[0].acq_eval(xq[0], 0.0), NO_GP % "pcabo_acq_eval")      # a member has no GP of its own yet
    res = bt.wpca_results()
    xq = [np.full((2, r["k"]), 0.25) for r in res]
    box = bt.acq_bounds()                              # allowed while the factorisation runs
    best = [float(v) for v in y.min(axis=1)]
    # ---- the scoring in two halves ----
    tok = bt.gp_eval_begin(xq, best)
    refused(lambda: bt.gp_eval_begin(xq, best), "pcabo_batch_gp_condition_end_eval: a scoring is already enqueued")
    refused(lambda: bt.gp_fit(), "pcabo_batch_gp_fit: a _begin call of this batch has not been ended")
    refused(lambda: bt.gp_posterior(xq), B_BUSY % "pcabo_batch_gp_posterior")
    vals, status = bt.gp_eval_end(tok)
    assert not status.any() and vals.shape == (B, 2)
    refused(lambda: bt.gp_eval_end(tok), "pcabo_batch_gp_condition_end_eval_end: no _begin before it")
    refused(lambda: bt.gp_wait_eval(xq, best), "pcabo_batch_gp_condition_end_eval: no conditioning in flight")
    refused(lambda: bt.gp_fit(), "pcabo_batch_gp_fit: call pcabo_batch_wpca_gp_condition_begin or pcabo_batch_gp_condition_begin first")
    # ---- conditioned ----
    assert all(p is not None for p in bt.gp_posterior(xq)) and all(p is not None for p in bt.gp_loo())
    assert bt.optimize_begin(xq, box, best) is None    # no refusal: the call does not qualify (test_batch_optimise_halves)
    refused(lambda: bt.optimize_end((2, 5)), "pcabo_batch_optimize_acqf_end: no matching _begin before it")
    outs, status = bt.optimize_acqf(xq, box, best)
    assert not status.any()
    z =[o[0][0] for o in outs]
    bt.inverse_map_begin(z)
    refused(lambda: bt.gp_posterior(xq), B_BUSY % "pcabo_batch_gp_posterior")
    x = bt.inverse_map_end()
    refused(lambda: bt.inverse_map_end(), "pcabo_batch_inverse_map_end: no _begin before it")
    assert np.array_equal(x, bt.inverse_map(z))
    # ---- a lock-step fit needs a conditioning in flight (or a fit before it) ----
    bt.wpca_gp_condition_begin(X, ranks, None, y)
    assert all(f["status"] == 0 for f in bt.gp_fit())
    assert all(f["status"] == 0 for f in bt.gp_fit())  # fitted: a second fit goes ahead
    vals, status = bt.gp_wait_eval(xq, best)           # ... and the fitted state is scored by the same call
    assert vals.shape == (B, 2)
    # ---- a member of a batch cannot be extended ----
    refused(lambda: bt.ctx[0].gp_extend(xq[0][:1], [0.0]), "pcabo_gp_extend: the context belongs to a batch")
    refused(lambda: bt.ctx[0].gp_truncate(3), "pcabo_gp_truncate: the context belongs to a batch")
    bt.close()


def test_batch_optimise_halves(native):
    """pcabo_batch_optimize_acqf_begin / _end need the device-resident optimiser, and that one a run's value buffer with room for
    a restart group's record behind its 64 values: max_q = 72 is the smallest batch they can be tried on."""
    B = 2
    X, y, ranks = data(B, 3)
    bt = native.Batch(B, max_n=8, max_d=2, max_q=72, device_lbfgsb=1)
    bt.wpca_gp_condition_begin(X, ranks, None, y)
    res = bt.wpca_results()
    xq = [np.full((2, r["k"]), 0.25) for r in res]
    box = bt.acq_bounds()
    best = [float(v) for v in y.min(axis=1)]
    refused(lambda: bt.optimize_begin(xq, box, best), "pcabo_batch_optimize_acqf_begin: no conditioned GP")
    assert not bt.gp_wait_eval(xq, best)[1].any()
    tok = bt.optimize_begin(xq, box, best)
    assert tok is not None, "the call did not qualify for the device optimiser"
    refused(lambda: bt.optimize_begin(xq, box, best), "pcabo_batch_optimize_acqf: an optimisation of this batch is already enqueued")
    refused(lambda: bt.optimize_acqf(xq, box, best), "pcabo_batch_optimize_acqf: an optimisation of this batch is already enqueued")
    refused(lambda: bt.gp_loo(), B_BUSY % "pcabo_batch_gp_loo")
    refused(lambda: bt.gp_fit(), "pcabo_batch_gp_fit: call pcabo_batch_wpca_gp_condition_begin or pcabo_batch_gp_condition_begin first")
    refused(lambda: bt.optimize_end((tok[0], tok[1] + 1)), "pcabo_batch_optimize_acqf_end: no matching _begin before it")
    outs, status = bt.optimize_end(tok)
    assert not status.any() and len(outs) == B
    refused(lambda: bt.optimize_end(tok), "pcabo_batch_optimize_acqf_end: no matching _begin before it")
    assert not bt.optimize_acqf(xq, box, best)[1].any()
    bt.close()


def test_single_context_calls_on_members(native):
    """A full lock-step iteration, then acq_eval, gp_state and gp_posterior on every member against a stand-alone context fed the
    same data: equal bytes at n = 3, and again after a second conditioning of the same batch and contexts at n = 4."""
    B = 2
    bt = native.Batch(B, max_n=8, max_d=2, max_q=16)
    alone = [native.Context(max_n=8, max_d=2, max_q=16) for _ in range(B)]
    for c in alone:
        c.set_option(native.OPT_GROUP_ACQ, 1)          # the batch's default kernel for value + gradient evaluations
    for n in (3, 4):
        X, y, ranks = data(B, n, seed=7)
        bt.wpca_gp_condition_begin(X, ranks, None, y)
        res = bt.wpca_results()
        box = bt.acq_bounds()
        xq = [box[b][0] + (box[b][1] - box[b][0]) * np.linspace(0.1, 0.9, 3 * res[b]["k"]).reshape(3, res[b]["k"]) for b in range(B)]
        best = [float(v) for v in y.min(axis=1)]
        vals, status = bt.gp_wait_eval(xq, best)
        assert not status.any()
        outs, status = bt.optimize_acqf(xq, box, best)
        assert not status.any()
        bt.inverse_map([o[0][0] for o in outs])
        for b in range(B):
            c, m = alone[b], bt.ctx[b]
            assert c.wpca_gp_condition(X[b], y[b], ranks=ranks[b])["k"] == res[b]["k"]
            c.gp_wait_eval(xq[b], best[b])
            sc, sm = c.gp_state(), m.gp_state()
            for key in ("L", "R", "alpha", "y_mean", "y_std", "norm_bounds"):
                assert np.array_equal(sc[key], sm[key]), (n, b, key)
            vc, gc = c.acq_eval(xq[b], best[b])
            vm, gm = m.acq_eval(xq[b], best[b])
            assert np.array_equal(vc, vm) and np.array_equal(gc, gm), (n, b)
            pc, pm = c.gp_posterior(xq[b], covariance=True), m.gp_posterior(xq[b], covariance=True)
            for key in ("mean", "variance", "covariance"):
                assert np.array_equal(pc[key], pm[key]), (n, b, key)
            refused(lambda: m.gp_extend(xq[b][:1], [0.0]), "pcabo_gp_extend: the context belongs to a batch")
    for c in alone:
        c.close()
    bt.close()
