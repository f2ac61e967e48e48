"""q candidates per iteration in the lock-step batches on the MI355X (BatchedPCABO / BatchedVanillaBO q=..., pcabo.batchrun
_later_proposals; pcabo_batch_acq_score).

  runs      every run of a batch with q = 3 (n_DoE 6, budget 13: 6 -> 9 -> 12 -> 13) holds, byte for byte, the points and values of
            the same seed alone with the same q, in "group" and in "latency" mode; "device" and "device-twin" agree with each
            other; a fitted batch with q = 2 equals the fitted single runs; the 64th row is filled inside the loop (62 -> 67).
  scoring   pcabo_batch_acq_score on an extended, unfitted batch - which pcabo_batch_gp_condition_end_eval refuses - gives every run
            the bytes Context.acq_eval(grad=False) gives it alone with the same extension, through the GEMM (q = 70) and through
            the per-query kernels (q = 3); a parked run is skipped, its block of the output untouched; the refusals.
  members   on an extended batch the single-context calls botorch's retry makes on a member - acq_eval and optimize_acqf - give the
            bytes of the run alone.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

from pcabo.bbob import BBOBProblem

pytestmark = pytest.mark.gpu

B, DIM, FID = 3, 5, 15
SEEDS = [15051 + i for i in range(B)]


@pytest.fixture(autouse=True)
def _full_sized(monkeypatch):
    monkeypatch.delenv("SMOKE_TEST", raising=False)


def _single(cls_name, seed, inst, n_doe, budget, **kw):
    import Algorithms
    opt = getattr(Algorithms, cls_name)(budget=budget, n_DoE=n_doe, random_seed=seed, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        opt(BBOBProblem(FID, inst, DIM))
    return np.vstack(opt.x_evals).tobytes(), np.array(opt.f_evals, dtype=np.float64).tobytes()


def _batched(cls_name, n_doe, budget, drive="run", **kw):
    from pcabo import batchrun
    r = getattr(batchrun, cls_name)([BBOBProblem(FID, i, DIM) for i in range(B)], SEEDS, budget, n_doe, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if drive == "run":
            r.run()
        else:
            batchrun.run_interleaved([r])
    assert all(f is None for f in r.failed)
    return r


def _bytes(r, b):
    return np.vstack(r.x_evals[b]).tobytes(), np.array(r.f_evals[b], dtype=np.float64).tobytes()


@pytest.mark.parametrize("batch_cls,single_cls,mode,single_kw", [
    ("BatchedPCABO", "PCA_BO", "group", {"acq_kernel": "group"}), ("BatchedPCABO", "PCA_BO", "latency", {}),
    ("BatchedVanillaBO", "Vanilla_BO", "latency", {})], ids=["pca-group", "pca-latency", "vanilla"])
@pytest.mark.parametrize("n_doe,budget", [(6, 13), (62, 67)])
def test_every_run_of_a_batch_is_the_run_alone(batch_cls, single_cls, mode, single_kw, n_doe, budget):
    r = _batched(batch_cls, n_doe, budget, acq_kernel=mode, q=3)
    for b in range(B):
        assert len(r.f_evals[b]) == budget
        assert _bytes(r, b) == _single(single_cls, SEEDS[b], b, n_doe, budget, q=3, **single_kw), b
    assert len(r.lbfgsb_info) == (7 if budget == 13 else 5)
    if (n_doe, budget) == (6, 13):
        one = _batched(batch_cls, n_doe, budget, acq_kernel=mode)
        assert any(_bytes(one, b) != _bytes(r, b) for b in range(B))              # q is not ignored


@pytest.mark.parametrize("strategy", ["constant_liar_min", "constant_liar_max"])
def test_liars_in_a_batch(strategy):
    r = _batched("BatchedPCABO", 6, 13, acq_kernel="latency", q=3, q_strategy=strategy, record_trace=True)
    for b in range(B):
        assert _bytes(r, b) == _single("PCA_BO", SEEDS[b], b, 6, 13, q=3, q_strategy=strategy), b
    assert sorted(len(t.get("proposals", [])) for t in r.trace) == [0] * B + [2] * (2 * B)


def test_device_and_its_twin_agree_and_interleaving_changes_nothing():
    dev = _batched("BatchedPCABO", 6, 13, acq_kernel="device", q=3)
    twin = _batched("BatchedPCABO", 6, 13, acq_kernel="device-twin", q=3)
    inter = _batched("BatchedPCABO", 6, 13, drive="interleaved", acq_kernel="device", q=3)
    for b in range(B):
        assert len(dev.f_evals[b]) == 13
        assert _bytes(dev, b) == _bytes(twin, b) == _bytes(inter, b), b


@pytest.mark.parametrize("batch_cls,single_cls", [("BatchedPCABO", "PCA_BO"), ("BatchedVanillaBO", "Vanilla_BO")])
def test_fitted_batch_with_q2(batch_cls, single_cls):
    r = _batched(batch_cls, 6, 11, acq_kernel="latency", q=2, fit_gp=True)
    for b in range(B):
        assert len(r.f_evals[b]) == 11
        assert _bytes(r, b) == _single(single_cls, SEEDS[b], b, 6, 11, q=2, fit_gp=True), b


# ---- pcabo_batch_acq_score and the member calls on an extended batch ----------------------------------------------------------
N, K, MAXQ = 40, 4, 128


def _data(seed=5):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-2.0, 2.0, (B, N, K))
    y = np.sin(Z.sum(axis=2)) * 3.0 + rng.normal(size=(B, N)) * 0.1 + 10.0
    Zp = rng.uniform(-2.0, 2.0, (B, 2, K))
    return Z, y, Zp


def _extended_batch(native, Z, y, Zp, parked=None):
    bt = native.Batch(B, max_n=64, max_d=K, max_q=MAXQ, group_acq=False)
    bt.gp_condition_begin(Z, y)
    probe = [Z[b][:3] for b in range(B)]
    _, status = bt.gp_wait_eval(probe, [float(y[b].min()) for b in range(B)])      # ends the conditioning: the batch is unfitted
    assert not status.any()
    if parked is not None:
        bt.set_active([b != parked for b in range(B)])
    n, status = bt.gp_extend([Zp[b] for b in range(B)])
    assert n == N + 2 and [int(s) for s in status] == [0 if b != parked else -1 for b in range(B)]
    return bt


def _alone(native, Z, y, Zp, b):
    c = native.Context(max_n=64, max_d=K, max_q=MAXQ)
    c.gp_condition(y[b], Z=Z[b])
    c.gp_extend(Zp[b])
    return c


@pytest.mark.parametrize("acq", ["EI", "PI", "UCB"])
def test_batch_acq_score_on_an_extended_unfitted_batch(native, acq):
    code = {"EI": native.ACQ_LOG_EI, "PI": native.ACQ_PI, "UCB": native.ACQ_UCB}[acq]
    Z, y, Zp = _data()
    bt = _extended_batch(native, Z, y, Zp, parked=1)
    rng = np.random.default_rng(9)
    scal = [float(np.float32(np.median(y[b]))) if acq != "UCB" else 1.5 for b in range(B)]
    try:
        for q in (70, 3):
            Xq = [rng.uniform(-2.2, 2.2, (q, K)) for _ in range(B)]
            with pytest.raises(native.PcaboError):                                # the scoring that ends a conditioning refuses
                bt.gp_wait_eval(Xq, scal, False, code)
            buf = np.zeros((B, q * K))
            for b in range(B):
                buf[b, : q * K] = Xq[b].ravel()
            val = np.full((B, q), -777.0)
            status = np.full(B, 99, dtype=np.int32)
            bf = np.array(scal)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            assert native.LIB.pcabo_batch_acq_score(bt._h, vp(buf), q, vp(bf), 0, code, vp(val), vp(status)) == 0
            assert [int(s) for s in status] == [0, -1, 0] and np.all(val[1] == -777.0)
            for b in (0, 2):
                c = _alone(native, Z, y, Zp, b)
                assert c.acq_eval(Xq[b], scal[b], False, code, grad=False).tobytes() == val[b].tobytes(), (q, b)
                c.close()
            v2, s2 = bt.acq_score(Xq, scal, False, code)                          # the binding, in halves
            assert v2[0].tobytes() == val[0].tobytes() and v2[2].tobytes() == val[2].tobytes() and list(s2) == [0, -1, 0]
        # refusals: a half that is open, bad arguments, no _begin
        tok = bt.acq_score_begin(Xq, scal, False, code)
        with pytest.raises(native.PcaboError):
            bt.acq_score_begin(Xq, scal, False, code)
        with pytest.raises(native.PcaboError):
            bt.gp_posterior(Xq)
        bt.acq_score_end(tok)
        with pytest.raises(native.PcaboError):
            bt.acq_score_end(tok)
        assert native.LIB.pcabo_batch_acq_score(bt._h, vp(buf), 0, vp(bf), 0, code, vp(val), vp(status)) == -1
        assert native.LIB.pcabo_batch_acq_score(bt._h, vp(buf), MAXQ + 1, vp(bf), 0, code, vp(val), vp(status)) == -1
        assert native.LIB.pcabo_batch_acq_score(bt._h, None, 3, vp(bf), 0, code, vp(val), vp(status)) == -1
        assert native.LIB.pcabo_batch_acq_score(bt._h, vp(buf), 3, vp(bf), 0, code, None, vp(status)) == -1
        assert native.LIB.pcabo_batch_acq_score(None, vp(buf), 3, vp(bf), 0, code, vp(val), vp(status)) == -1
        assert bt.gp_truncate() == N
    finally:
        bt.close()
    fresh = native.Batch(B, max_n=64, max_d=K, max_q=MAXQ)
    try:
        with pytest.raises(native.PcaboError):                                    # no GP yet
            fresh.acq_score([Z[b][:3] for b in range(B)], scal, False, code)
        fresh.gp_condition_begin(Z, y)
        with pytest.raises(native.PcaboError):                                    # a conditioning that has not been waited for
            fresh.acq_score([Z[b][:3] for b in range(B)], scal, False, code)
        vals, status = fresh.gp_wait_eval([Z[b][:3] for b in range(B)], scal, False, code)       # ... still ends as before
        again, _ = fresh.acq_score([Z[b][:3] for b in range(B)], scal, False, code)              # and the model is scored as it stands
        assert not status.any() and again.tobytes() == vals.tobytes()
    finally:
        fresh.close()


@pytest.mark.parametrize("group", [False, True])
def test_member_calls_on_an_extended_batch(native, group):
    """What `_retry` does on `Batch.ctx[b]` while the batch is extended: scoring and one optimiser call, as the run alone."""
    Z, y, Zp = _data(seed=6)
    bt = native.Batch(B, max_n=64, max_d=K, max_q=MAXQ, group_acq=group)
    try:
        bt.gp_condition_begin(Z, y)
        best = [float(np.float32(y[b].min())) for b in range(B)]
        bt.gp_wait_eval([Z[b][:3] for b in range(B)], best)
        bt.gp_extend([Zp[b] for b in range(B)])
        rng = np.random.default_rng(4)
        box = np.array([[-2.0] * K, [2.0] * K])
        for b in range(B):
            Xq, ics = rng.uniform(-2.0, 2.0, (70, K)), rng.uniform(-2.0, 2.0, (6, K))
            c = _alone(native, Z, y, Zp, b)
            c.set_option(native.OPT_GROUP_ACQ, int(group))
            m = bt.ctx[b]
            assert m.acq_eval(Xq, best[b], grad=False).tobytes() == c.acq_eval(Xq, best[b], grad=False).tobytes()
            got, want = m.optimize_acqf(ics, box, best[b], batch_limit=3), c.optimize_acqf(ics, box, best[b], batch_limit=3)
            assert all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want)), b
            c.close()
    finally:
        bt.close()
