"""sha256 of what the posterior entry points return - mean, variance, covariance, samples and the rung of the jitter ladder - on
the smallest states that reach each form of their kernels (the score GEMM with and without the store of V, k_post_combine,
k_post_cov, k_post_chol_prep, k_post_sample) and each half of the ladder:
  s{i}_plain / s{i}_nasty   Context: row i of posterior_samples_reference.SHAPES with its plain and its nasty queries; gp_posterior
                            with the covariance, then gp_posterior_samples on the base of seed q + S
  k70_plain / k70_nasty     n = 130, k = 70, q = 65: the coordinate loop of k_post_cov takes a second 64-wide pass
  s3_nasty_centred          centred samples (the ladder climbs: a duplicate row, no observation noise)
  s4_plain_mean_var         a query without the covariance: the score GEMM that stores no V
  batch3_{cond,fit}         Batch of 3 runs with different k, run 1 parked, before and after the lock-step fit (the data of
                            test_batch_equals_alone); run 2 has nasty queries, so without observation noise it climbs the ladder
                            alone while run 0 factors on the first rung
  batch1                    a one-run batch on row 3 of SHAPES, nasty queries
compute() asserts that a context case and the lone batch run do climb.  tests/golden/posterior_hashes.json holds the bits of the
library before the tile product and the host sequence of the posterior were written once each (PCABO_LIB selects the library).
    python tools/gpu_posterior_hashes.py            # print
    python tools/gpu_posterior_hashes.py --write    # regenerate (only after an INTENDED change of arithmetic)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "para-ortho-pca-bo_amd"):
    if os.path.join(ROOT, p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
from ard_reference import ard_state
from posterior_samples_reference import KERNEL, RUNGS, SHAPES, base_samples, nasty_queries, plain_queries, state

GOLDEN = os.path.join(ROOT, "tests", "golden", "posterior_hashes.json")
K70 = (130, 70, 65, 3, "matern52", False, False)             # a row in the form of SHAPES
QUERIES = {"plain": plain_queries, "nasty": nasty_queries}
B, N, D, Q, S_B, LO = 3, 130, 9, 130, 65, (1.0, 0.3, 0.05)   # the batch of tests/test_gpu_posterior_samples.py


def _h(a) -> str:
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert np.isfinite(a).all()
    return hashlib.sha256(a.tobytes()).hexdigest()


def _record(post, smp) -> dict:
    """The hashes of a query and of the samples at the same points; the rung also in the clear."""
    assert smp["jitter"] in RUNGS
    rec = {key: _h(post[key]) for key in ("mean", "variance", "covariance") if key in post}
    rec.update(samples=_h(smp["samples"]), sample_mean=_h(smp["mean"]), jitter=_h(smp["jitter"]), rung=smp["jitter"])
    return rec


def context_cases(N_) -> dict:
    ctx = N_.Context(max_n=257, max_d=70, max_q=192)
    out = {}

    def case(shape, what, covariance=True, centred=False):
        n, k, q, S, kernel, noise = shape[:6]
        Z, y = ard_state(500 + n + k, n, k) if shape is K70 else state(shape)[:2]
        nb = None if shape is K70 else state(shape)[2]
        Xq = QUERIES[what](Z, q, n + q)
        ctx.gp_condition(y, Z=Z, norm_bounds=nb, kernel=KERNEL[kernel])
        post = ctx.gp_posterior(Xq, observation_noise=noise, covariance=covariance)
        return _record(post, ctx.gp_posterior_samples(Xq, base_samples=base_samples(q, S), observation_noise=noise, centred=centred))

    for i, shape in enumerate(SHAPES):
        for what in QUERIES:
            out["s%d_%s" % (i, what)] = case(shape, what)
    for what in QUERIES:
        out["k70_" + what] = case(K70, what)
    out["s3_nasty_centred"] = case(SHAPES[3], "nasty", centred=True)
    out["s4_plain_mean_var"] = case(SHAPES[4], "plain", covariance=False)
    ctx.close()
    assert any(rec["rung"] != 0.0 for rec in out.values()) and out["s3_nasty_centred"]["rung"] != 0.0
    assert "covariance" not in out["s4_plain_mean_var"]
    return out


def _batch_state(b):
    rng = np.random.default_rng(21 + b)
    X = rng.uniform(-5, 5, (N, D)) * np.linspace(1, LO[b], D)
    y = np.sin(0.7 * X[:, 0]) * 40 + (X ** 2).sum(1) + rng.normal(size=N)
    return X, y, rng.normal(0, 1e-8, X.shape)


def batch3_case(N_, fitted) -> dict:
    X, y, noise = (np.stack(a) for a in zip(*[_batch_state(b) for b in range(B)]))
    ranks = np.argsort(np.argsort(y, axis=1), axis=1).astype(np.int64) + 1
    bt = N_.Batch(B, max_n=N, max_d=D, max_q=Q)
    bt.wpca_gp_condition_begin(X, ranks, noise, y)
    ks = [r["k"] for r in bt.wpca_results()]
    assert len(set(ks)) >= 2, ks
    boxes = bt.acq_bounds()
    Xq = [np.random.default_rng(40 + b).uniform(boxes[b][0], boxes[b][1], size=(Q, ks[b])) for b in range(B)]
    Xq[2][1], Xq[2][Q - 1] = Xq[2][0] + 1e-9, Xq[2][3]       # run 2: two points 1e-9 apart and a duplicate row
    base = np.stack([np.random.default_rng(60 + b).standard_normal((S_B, Q)) for b in range(B)])
    if fitted:
        bt.gp_fit()
    else:
        assert not bt.gp_wait_eval(Xq, y.min(axis=1))[1].any()
    bt.set_active([1, 0, 1])
    out = {"k": ks}
    for noisy, centred in ((False, False), (True, True)):
        post = bt.gp_posterior(Xq, observation_noise=noisy, covariance=True)
        smp = bt.gp_posterior_samples(Xq, base_samples=base, observation_noise=noisy, centred=centred)
        assert post[1] is None and smp[1] is None and list(bt.sample_status) == [0, -1, 0]
        for b in (0, 2):
            out["run%d_noise%d" % (b, noisy)] = _record(post[b], smp[b])
    bt.close()
    assert out["run0_noise0"]["rung"] == 0.0 and out["run2_noise0"]["rung"] != 0.0      # run 2 climbs alone
    return out


def batch1_case(N_) -> dict:
    shape = SHAPES[3]
    n, k, q, S, kernel, noise = shape[:6]
    Z, y, _ = state(shape)
    Xq = nasty_queries(Z, q, n + q)
    bt = N_.Batch(1, max_n=n, max_d=k, max_q=q)
    bt.gp_condition_begin(Z[None], y[None], kernel=KERNEL[kernel])
    assert not bt.gp_wait_eval([Xq], [float(y.min())])[1].any()
    post = bt.gp_posterior([Xq], observation_noise=noise, covariance=True)
    smp = bt.gp_posterior_samples([Xq], base_samples=base_samples(q, S), observation_noise=noise)
    bt.close()
    return _record(post[0], smp[0])


def compute() -> dict:
    from pcabo import _native as N_
    out = context_cases(N_)
    out["batch3_cond"], out["batch3_fit"] = batch3_case(N_, False), batch3_case(N_, True)
    out["batch1"] = batch1_case(N_)
    return out


if __name__ == "__main__":
    res = compute()
    if "--write" in sys.argv:
        i = sys.argv.index("--write")
        out = sys.argv[i + 1] if len(sys.argv) > i + 1 else GOLDEN
        with open(out, "w") as f:
            json.dump({"_comment": "tools/gpu_posterior_hashes.py --write on an MI355X, with the library of commit 2c7a75f: before "
                                   "the posterior's tile product and host sequence were written once each", "cases": res}, f, indent=1)
        print("written", out)
    else:
        print(json.dumps(res, indent=1))
