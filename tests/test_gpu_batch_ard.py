"""The lock-step ARD fit of a batch on the MI355X (pcabo_batch_gp_mll_ard / pcabo_batch_gp_fit_ard: k_zstats with per-run
lengthscales and fold switch, k_mll_grad<true> / k_mll_finish<true> with grid z = B; Batch.gp_mll_ard / Batch.gp_fit_ard,
BatchedPCABO / BatchedVanillaBO fit_gp=True, batched_ard=True, ExperimentRunner batched_fit_gp=True, batched_ard=True).

Every run of a batch must take, bit for bit, the evaluations, the fit and the path the same run takes alone through
pcabo_gp_mll_ard / pcabo_gp_fit_ard; one test holds the batch directly to the restatement of tests/ard_reference.py with the caps
of tests/test_gpu_ard.py, so that an error shared by batch and single context would show.

The states: ard_state(seed, n, k) of tests/ard_reference.py laid into the first k of D = 9 coordinates, the other coordinates at
1e-4 of their scale, so that the weighted PCA with var_threshold 0.999 keeps exactly k components (every kept component holds more
than 1 / 30 of the variance, the dropped ones 1e-9 each) - the runs of one batch then have k = (9, 5, 3, 1): KP = 12, 8, 4, 4,
the eight-wide input walk of k_mll_grad<true> with a ragged second trip, and a run with a single input beside wider ones.
n = 65: NP = 128, three tiles, one of them off-diagonal, ragged rows; n = 40: one tile; B = 9: past one XCD group of the
conditioning kernels' placement.

The seeds of the fitted batches were chosen on the CPU: the restated fits ArdFit.fit(rho_min=RHO_MIN) of the reduced states with
seeds (11, 12, 13, 14) at n = 65 take 245 / 108 / 62 / 47 evaluations, those of the Vanilla-style states (21 .. 24, k = 4) take
116 / 106 / 93 / 199, so the runs of a batch cannot all finish in one round (the k = 9 reference fit alone takes 13 s of CPU time,
so it is not repeated here; the device tests assert min < max on the device's own counts)."""
import os

import numpy as np
import pytest
import torch

from ard_reference import ArdFit, ard_state, theta0
from pcabo.bbob import BBOBProblem

pytestmark = pytest.mark.gpu

LOSS_CAP, GRAD_CAP = 1e-9, 1e-7                                     # tests/test_gpu_ard.py
D, VT = 9, 0.999
KS = (9, 5, 3, 1)
SEEDS = (11, 12, 13, 14)
KS9, SEEDS9 = KS + KS + (2,), SEEDS + (15, 16, 17, 18, 19)
FIT_KEYS = ("iterations", "evaluations", "warnflag", "task")
STATE_KEYS = ("L", "R", "alpha", "norm_bounds")


def embedded_state(seed, n, k):
    """ard_state(seed, n, k) in the first k of D coordinates: (X, y, noise, ranks) as the weighted PCA takes them."""
    Z, y = ard_state(seed, n, k)
    rng = np.random.default_rng(9000 + seed)
    X = 1e-4 * rng.uniform(-2.0, 2.0, size=(n, D))
    X[:, :k] = Z
    noise = rng.normal(0, 1e-8, X.shape)
    return X, y, noise, np.argsort(np.argsort(y)).astype(np.int64) + 1


def batch_data(n, ks=KS, seeds=SEEDS):
    return tuple(np.stack(a) for a in zip(*[embedded_state(s, n, k) for s, k in zip(seeds, ks)]))


def thetas_for(k, seed):
    """The five thetas of tests/test_gpu_ard.py: the start; seeded rho in [-1.5, 2] with c != 0; the noise at its bound; one
    rho_c = 15; one rho_c = 25 (softplus's linear branch)."""
    rng = np.random.default_rng(1000 * seed + k)
    rho = rng.uniform(-1.5, 2.0, size=k)
    c = int(rng.integers(k))
    big, lin = rho.copy(), rho.copy()
    big[c], lin[c] = 15.0, 25.0
    return [theta0(k), np.r_[0.05, 0.3, rho], np.r_[1e-4, -0.2, rho], np.r_[0.05, 0.3, big], np.r_[0.02, -0.1, lin]]


def _batch(native, data, max_q=512):
    """A batch with its conditioning in flight on `data`, the wPCA results collected."""
    X, y, noise, ranks = data
    bt = native.Batch(X.shape[0], max_n=X.shape[1], max_d=D, max_q=max_q)
    bt.wpca_gp_condition_begin(X, ranks, noise, y, var_threshold=VT)
    return bt, bt.wpca_results()


def _alone(native, data, b, max_q=512):
    """A fresh stand-alone context holding run b's own weighted PCA (as PCA_BO(fit_gp=True, ard=True) runs it)."""
    X, y, noise, ranks = data
    c = native.Context(max_n=X.shape[1], max_d=D, max_q=max_q)
    return c, c.wpca(X[b], ranks=ranks[b], noise=noise[b], var_threshold=VT)


def _same_state(a, b):
    return all(a[key].tobytes() == b[key].tobytes() for key in STATE_KEYS)


def _same_fit(a, b):
    return (a["theta"].tobytes() == b["theta"].tobytes() and a["loss"] == b["loss"] and all(a[key] == b[key] for key in FIT_KEYS))


# ---- 1. one evaluation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["n65", "n65-parked", "n40", "n65-B9"])
def test_batch_gp_mll_ard_equals_the_single_context_bit_for_bit(native, shape):
    n = 40 if shape == "n40" else 65
    ks, seeds = (KS9, SEEDS9) if shape.endswith("B9") else (KS, SEEDS)
    parked = 1 if shape.endswith("parked") else None
    data = batch_data(n, ks, seeds)
    B = len(ks)
    bt, res = _batch(native, data)
    singles = []
    try:
        assert [r["k"] for r in res] == list(ks)
        if parked is not None:
            bt.set_active([b != parked for b in range(B)])
            scalar = bt.gp_mll(np.tile([0.05, 0.3, 0.2], (B, 1)))
            assert scalar[parked] == {"status": -1}
            parked_slab = bt.ctx[parked].gp_state()       # what the scalar round leaves for a parked run: the shared, unfolded model
        for b in range(B):
            c, r1 = _alone(native, data, b)
            singles.append(c)
            assert r1["k"] == ks[b]
        per_run = [thetas_for(ks[b], seeds[b]) for b in range(B)]
        for i in range(5):
            thetas = [per_run[b][(i + b) % 5] for b in range(B)]           # another kind of theta per run in every call
            out = bt.gp_mll_ard(thetas)
            assert bt.fit_rounds == 1
            for b in range(B):
                if b == parked:
                    assert out[b] == {"status": -1}
                    assert _same_state(bt.ctx[b].gp_state(), parked_slab)
                    continue
                one = singles[b].gp_mll_ard(data[1][b], thetas[b])
                assert out[b]["status"] == 0
                assert out[b]["loss"] == one["loss"], (shape, i, b, out[b]["loss"], one["loss"])
                assert out[b]["grad"].shape == (2 + ks[b],) and out[b]["grad"].tobytes() == one["grad"].tobytes(), (shape, i, b)
                assert out[b]["theta"].tobytes() == one["theta"].tobytes() == np.asarray(thetas[b]).tobytes()
                assert out[b]["lengthscales"].tobytes() == one["lengthscales"].tobytes()
                assert _same_state(bt.ctx[b].gp_state(), singles[b].gp_state()), (shape, i, b)
    finally:
        bt.close()
        for c in singles:
            c.close()


# ---- 5. the batch against the restatement (not only against the single context) ----------------------------------------------
def test_batch_gp_mll_ard_matches_the_restated_loss_and_gradient(native, capsys):
    data = batch_data(65)
    bt, res = _batch(native, data)
    worst_l = worst_g = 0.0
    try:
        refs = []
        for b in range(len(KS)):
            c, r1 = _alone(native, data, b)                   # (the reduced points: the context's own weighted PCA)
            c.close()
            assert r1["k"] == res[b]["k"] == KS[b]
            refs.append(ArdFit(r1["Z"], data[1][b]))
        per_run = [thetas_for(KS[b], SEEDS[b]) for b in range(len(KS))]
        for i in range(5):
            thetas = [per_run[b][(i + b) % 5] for b in range(len(KS))]
            out = bt.gp_mll_ard(thetas)
            for b, ref in enumerate(refs):
                lv, lg = ref.value_and_grad(thetas[b])
                el = abs(out[b]["loss"] - lv) / max(abs(lv), 1e-2)
                eg = np.abs(out[b]["grad"] - lg) / np.maximum(np.abs(lg), 1e-3 * ref.term_scales(thetas[b]))
                print(f"  theta set {i}, run {b} (k = {KS[b]}): loss {el:.2e}, gradient {eg.max():.2e} (component {int(eg.argmax())})")
                worst_l, worst_g = max(worst_l, el), max(worst_g, float(eg.max()))
                assert el <= LOSS_CAP, (i, b, out[b]["loss"], lv)
                assert (eg <= GRAD_CAP).all(), (i, b, int(eg.argmax()), out[b]["grad"][eg.argmax()], lg[eg.argmax()])
    finally:
        bt.close()
    with capsys.disabled():
        print(f"\n  Batch.gp_mll_ard vs restatement at n = 65, k = {KS}: loss {worst_l:.2e} (cap {LOSS_CAP:.0e}), "
              f"gradient {worst_g:.2e} (cap {GRAD_CAP:.0e})")


# ---- 2. and 3. the fit, and the fitted batch ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(native):
    """The n = 65, k = (9, 5, 3, 1) batch after Batch.gp_fit_ard, and one context per run after Context.gp_fit_ard (shared, unchanged
    by the tests: they only query)."""
    data = batch_data(65)
    bt, res = _batch(native, data)
    singles, one = [], []
    fits = bt.gp_fit_ard()
    rounds = bt.fit_rounds
    for b in range(len(KS)):
        c, r1 = _alone(native, data, b)
        singles.append(c)
        one.append(c.gp_fit_ard(data[1][b]))
    yield data, bt, fits, rounds, singles, one
    bt.close()
    for c in singles:
        c.close()


def test_batch_gp_fit_ard_equals_the_single_fits_bit_for_bit(native, fitted, capsys):
    data, bt, fits, rounds, singles, one = fitted
    for b in range(len(KS)):
        assert fits[b]["status"] == 0
        assert fits[b]["theta"].shape == (2 + KS[b],) and fits[b]["lengthscales"].shape == (KS[b],)
        assert _same_fit(fits[b], one[b]), (b, fits[b], one[b])
        assert _same_state(bt.ctx[b].gp_state(), singles[b].gp_state()), b
    evals = [f["evaluations"] for f in fits]
    assert min(evals) < max(evals), evals                   # the runs do not all finish in one round: finished ones rest
    assert rounds >= max(evals)
    with capsys.disabled():
        print(f"\n  lock-step ARD fit, k = {KS}: evaluations {evals}, iterations {[f['iterations'] for f in fits]}, "
              f"warnflags {[f['warnflag'] for f in fits]}, {rounds} rounds")


def test_two_fits_of_one_batch_state_and_a_larger_batch_are_bit_identical(native, fitted):
    data, _, first, _, _, _ = fitted
    bt, _ = _batch(native, data)
    try:
        a, b = bt.gp_fit_ard(), bt.gp_fit_ard()
    finally:
        bt.close()
    order = [0, 1, 2, 3, 3, 2, 1, 0]
    big, res = _batch(native, tuple(x[order] for x in data))
    try:
        assert [r["k"] for r in res] == [KS[j] for j in order]
        wide = big.gp_fit_ard()
    finally:
        big.close()
    for j in range(len(KS)):
        assert _same_fit(first[j], a[j]) and _same_fit(a[j], b[j]), j
    for j, src in enumerate(order):
        assert _same_fit(first[src], wide[j]), (j, src)


def test_vanilla_style_batch_gp_fit_ard_equals_the_single_fits(native):
    """pcabo_batch_gp_condition_begin with identity Normalize bounds (BatchedVanillaBO): equal k, the fit on the raw points."""
    n, k, seeds = 65, 4, (21, 22, 23, 24)
    states = [ard_state(s, n, k) for s in seeds]
    Zs = np.stack([Z / 4.0 + 0.5 for Z, _ in states])       # the raw points in the unit box
    y = np.stack([v for _, v in states])
    ident = np.vstack([np.zeros(k), np.ones(k)])
    bt = native.Batch(len(seeds), max_n=n, max_d=k, max_q=64)
    c = native.Context(max_n=n, max_d=k, max_q=64)
    try:
        bt.gp_condition_begin(Zs, y, norm_bounds=ident)
        fits = bt.gp_fit_ard()
        for b in range(len(seeds)):
            one = c.gp_fit_ard(y[b], Z=Zs[b], norm_bounds=ident)
            assert fits[b]["status"] == 0 and _same_fit(fits[b], one), (b, fits[b], one)
            assert _same_state(bt.ctx[b].gp_state(), c.gp_state()), b
        evals = [f["evaluations"] for f in fits]
        assert min(evals) < max(evals) and bt.fit_rounds >= max(evals), (evals, bt.fit_rounds)
    finally:
        bt.close()
        c.close()


def test_after_the_fit_batch_and_alone_agree_bit_for_bit(native, fitted):
    data, bt, fits, _, singles, _ = fitted
    y = data[1]
    B = len(KS)
    boxes = bt.acq_bounds()
    for b in range(B):
        assert np.array_equal(boxes[b], singles[b].acq_bounds()), b                  # the search box is never folded
    Xq = [np.random.default_rng(40 + b).uniform(boxes[b][0], boxes[b][1], size=(64, KS[b])) for b in range(B)]
    for noisy in (False, True):
        out = bt.gp_posterior(Xq, observation_noise=noisy, covariance=True)
        for b in range(B):
            alone = singles[b].gp_posterior(Xq[b], observation_noise=noisy, covariance=True)
            assert out[b] is not None
            assert all(out[b][key].tobytes() == alone[key].tobytes() for key in ("mean", "variance", "covariance")), (b, noisy)
    raw = [np.random.default_rng(60 + b).uniform(boxes[b][0], boxes[b][1], size=(512, KS[b])) for b in range(B)]
    best = [float(y[b].min()) for b in range(B)]
    kappa = [float(np.sqrt(2.0))] * B
    for scalars, code in ((best, native.ACQ_LOG_EI), (kappa, native.ACQ_UCB)):
        vals, status = bt.gp_wait_eval(raw, scalars, False, code)
        assert not status.any()
        for b in range(B):
            alone = singles[b].acq_eval(raw[b], scalars[b], False, code, grad=False)
            assert vals[b].tobytes() == np.asarray(alone).tobytes(), (b, code)


def test_the_next_conditioning_returns_to_the_unfolded_shared_model(native):
    """(On given points, without the weighted PCA: its eigen-solver starts from the last call's vectors, so a second wPCA of one
    batch need not give the first one's bits, fit or no fit.)"""
    n, k, seeds = 65, 3, (31, 32, 33)
    states = [ard_state(s, n, k) for s in seeds]
    Z, y = np.stack([s[0] for s in states]), np.stack([s[1] for s in states])
    bt = native.Batch(len(seeds), max_n=n, max_d=k, max_q=64)
    fresh = native.Batch(len(seeds), max_n=n, max_d=k, max_q=64)
    try:
        bt.gp_condition_begin(Z, y)
        fits = bt.gp_fit_ard()
        for b in range(len(seeds)):                             # folded: lo as it was, the range times the run's lengthscales
            lo, hi = Z[b].min(0), Z[b].max(0)
            nb = bt.ctx[b].gp_state()["norm_bounds"]
            assert np.allclose(nb[0], lo - 0.1 * (hi - lo), rtol=1e-15, atol=0)
            assert np.allclose(nb[1] - nb[0], 1.2 * (hi - lo) * fits[b]["lengthscales"], rtol=1e-13, atol=0)
        bt.gp_condition_begin(Z, y)
        fresh.gp_condition_begin(Z, y)
        boxes = fresh.acq_bounds()
        Xq = [np.random.default_rng(5 + b).uniform(boxes[b][0], boxes[b][1], size=(64, k)) for b in range(len(seeds))]
        va, sa = bt.gp_wait_eval(Xq, y.min(axis=1))
        vb, sb = fresh.gp_wait_eval(Xq, y.min(axis=1))
        assert not sa.any() and not sb.any() and va.tobytes() == vb.tobytes()
        for b in range(len(seeds)):
            assert _same_state(bt.ctx[b].gp_state(), fresh.ctx[b].gp_state()), b
    finally:
        bt.close()
        fresh.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(native):
    data = batch_data(40)
    X, y, noise, ranks = data
    B = len(KS)
    bt = native.Batch(B, max_n=40, max_d=D, max_q=64)
    try:
        for call in (lambda: bt.gp_mll_ard(None), lambda: bt.gp_fit_ard()):          # nothing conditioned: the runs' k are unknown
            with pytest.raises(ValueError):
                call()
        bt.wpca_gp_condition_begin(X, ranks, noise, y, var_threshold=VT, kernel=native.KERNEL_RBF)
        bt.wpca_results()
        for call in (lambda: bt.gp_mll_ard(None), lambda: bt.gp_fit_ard()):          # RBF
            with pytest.raises(native.PcaboError) as e:
                call()
            assert e.value.code == -1
    finally:
        bt.close()
    bt = native.Batch(B, max_n=40, max_d=D, max_q=64)
    try:
        bt.k = np.array(KS, dtype=np.int32)                     # (the binding's own check aside) no conditioning in flight
        for call in (lambda: bt.gp_mll_ard(None), lambda: bt.gp_fit_ard()):
            with pytest.raises(native.PcaboError) as e:
                call()
            assert e.value.code == -1
        bt.wpca_gp_condition_begin(X, ranks, noise, y, var_threshold=VT)
        bt.wpca_results()
        C = native.C
        th = np.zeros((B, 2 + max(KS)))
        th[:, 0] = 0.01
        loss, grad = np.zeros(B), np.zeros_like(th)
        info, status = np.zeros((B, 4), dtype=np.int32), np.zeros(B, dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)            # noqa: E731
        for ld in (0, 3, 1 + max(KS)):                          # ld_theta below 2 + max k
            assert native.LIB.pcabo_batch_gp_mll_ard(bt._h, ptr(th), ld, ptr(loss), ptr(grad), ptr(status)) == -1
            assert native.LIB.pcabo_batch_gp_fit_ard(bt._h, ptr(th), ld, ptr(loss), ptr(info), ptr(status)) == -1
            assert "ld_theta" in bt._err()
        # a theta outside the model's domain: that run's status is set, the others go on
        thetas = [theta0(k) for k in KS]
        good = bt.gp_mll_ard(thetas)
        for bad in (np.r_[0.0, 0.0, np.zeros(KS[1])], np.r_[0.01, 0.0, np.full(KS[1], -800.0)], np.r_[0.01, float("nan"), np.zeros(KS[1])]):
            out = bt.gp_mll_ard([thetas[0], bad, thetas[2], thetas[3]])
            assert out[1] == {"status": -1}
            for b in (0, 2, 3):
                assert out[b]["status"] == 0 and out[b]["loss"] == good[b]["loss"] and out[b]["grad"].tobytes() == good[b]["grad"].tobytes()
        fits = bt.gp_fit_ard([thetas[0], np.r_[0.01, 0.0, np.full(KS[1], -800.0)], thetas[2], thetas[3]])
        assert fits[1] == {"status": -1} and all(fits[b]["status"] == 0 for b in (0, 2, 3))
        # a member context's own ARD calls stay refused
        for call in (lambda: bt.ctx[3].gp_mll_ard(y[3], theta0(1)), lambda: bt.ctx[3].gp_fit_ard(y[3])):
            with pytest.raises(native.PcaboError) as e:
                call()
            assert e.value.code == -1
    finally:
        bt.close()


# ---- 4. whole runs ---------------------------------------------------------------------------------------------------------
def _equal_runs(r, b, opt):
    assert np.array_equal(np.vstack(r.x_evals[b]), np.vstack(opt.x_evals)), b
    assert np.array_equal(np.array(r.f_evals[b]), np.array(opt.f_evals)), b
    assert r.current_best[b] == opt.current_best and r.current_best_index[b] == opt.current_best_index
    hb, h1 = r.gp_hyperparameters[b], opt.gp_hyperparameters
    assert hb["theta"].tobytes() == h1["theta"].tobytes() and hb["lengthscales"].tobytes() == h1["lengthscales"].tobytes(), b
    assert hb["loss"] == h1["loss"] and all(hb[key] == h1[key] for key in FIT_KEYS), b


@pytest.mark.parametrize("mode", ["group", "latency"])
def test_batched_pca_runs_with_batched_ard_equal_single_runs_bit_for_bit(native, mode):
    from Algorithms import PCA_BO
    from pcabo.batchrun import BatchedPCABO
    torch.set_num_threads(4)
    dim, budget, n_doe, runs = 10, 70, 60, 4                # n crosses the tile boundary 64 within the ten iterations
    seeds = [15000 + 10 * dim + i for i in range(runs)]
    r = BatchedPCABO([BBOBProblem(15, i, dim) for i in range(runs)], seeds, budget, n_doe, acq_kernel=mode, fit_gp=True,
                     batched_ard=True)
    r.run()
    assert r.timing["fit"] > 0.0 and all(f is None for f in r.failed)
    for b in range(runs):
        opt = PCA_BO(budget=budget, n_DoE=n_doe, random_seed=seeds[b], maximization=False, acq_kernel=mode, fit_gp=True, ard=True)
        opt(BBOBProblem(15, b, dim))
        _equal_runs(r, b, opt)


def test_batched_vanilla_runs_with_batched_ard_equal_single_runs_bit_for_bit(native):
    from Algorithms import Vanilla_BO
    from pcabo.batchrun import BatchedVanillaBO
    torch.set_num_threads(4)
    fid, dim, budget, n_doe, runs = 15, 10, 70, 60, 4
    seeds = [1000 * fid + 10 * dim + i for i in range(runs)]
    r = BatchedVanillaBO([BBOBProblem(fid, i, dim) for i in range(runs)], seeds, budget, n_doe, acq_kernel="latency", fit_gp=True,
                         batched_ard=True)
    r.run()
    assert r.timing["fit"] > 0.0 and all(f is None for f in r.failed)
    for b in range(runs):
        opt = Vanilla_BO(budget=budget, n_DoE=n_doe, random_seed=seeds[b], maximization=False, fit_gp=True, ard=True)
        opt(BBOBProblem(fid, b, dim))
        _equal_runs(r, b, opt)


def test_device_stepping_equals_its_twin_with_batched_ard(native):
    from pcabo.batchrun import BatchedPCABO, device_mode_covers
    dim, budget, n_doe, runs = 5, 30, 20, 3                 # small: device_mode_covers holds for every budget <= 512, dim <= 40
    assert device_mode_covers(dim, budget)
    seeds = [15000 + 10 * dim + i for i in range(runs)]
    out = {}
    for mode in ("device", "device-twin"):
        r = BatchedPCABO([BBOBProblem(15, i, dim) for i in range(runs)], seeds, budget, n_doe, acq_kernel=mode, fit_gp=True,
                         batched_ard=True)
        r.run()
        assert all(f is None for f in r.failed)
        out[mode] = r
    for b in range(runs):
        assert np.array_equal(np.vstack(out["device"].x_evals[b]), np.vstack(out["device-twin"].x_evals[b])), b
        assert np.array_equal(np.array(out["device"].f_evals[b]), np.array(out["device-twin"].f_evals[b])), b
        hd, ht = out["device"].gp_hyperparameters[b], out["device-twin"].gp_hyperparameters[b]
        assert hd["theta"].tobytes() == ht["theta"].tobytes() and "lengthscales" in hd


def test_experiment_runner_batched_ard_writes_the_same_files(native, tmp_path):
    from Algorithms import ExperimentRunner
    outs = []
    for batched in (0, 3):
        root = tmp_path / f"b{batched}"
        kw = dict(batched=3, batched_fit_gp=True, batched_ard=True, batch_acq_kernel="latency") if batched \
            else dict(batched=0, fit_gp=True, ard=True)
        er = ExperimentRunner(algorithms=["pca"], dimensions=[5], problem_ids=[15, 20], num_runs=3, budget_factor=5,
                              doe_factor=2.0, root_dir=str(root), experiment_name="experiment", progress=False, **kw)
        er.run_experiment()
        assert len(er.results) == 6
        outs.append((root, sorted((r["problem_id"], r["instance"], r["best"]) for r in er.results)))
    assert outs[0][1] == outs[1][1]
    for fid, name in ((15, "RastriginRotated"), (20, "Schwefel")):
        rel = os.path.join("pca-experiment", f"data_f{fid}_{name}", f"IOHprofiler_f{fid}_DIM5.dat")
        a, b = open(os.path.join(outs[0][0], rel)).read(), open(os.path.join(outs[1][0], rel)).read()
        assert a == b
    for root, _ in outs:
        meta = open(os.path.join(root, "pca-experiment", "IOHprofiler_f15_RastriginRotated.json")).read()
        assert '"gp_fit": "map-ard"' in meta
