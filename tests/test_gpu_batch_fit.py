"""The lock-step GP hyperparameter fit of a batch on the MI355X (pcabo_batch_gp_mll / pcabo_batch_gp_fit, Batch.gp_mll /
Batch.gp_fit, BatchedPCABO / BatchedVanillaBO fit_gp=True, ExperimentRunner batched_fit_gp=True).

Every run of a batch must take, bit for bit, the evaluations, the fit and the path the same run takes alone through
pcabo_gp_mll / pcabo_gp_fit (Context.gp_mll / Context.gp_fit, PCA_BO / Vanilla_BO fit_gp=True); against the restatement of
tests/test_gp_fit_cpu.py (torch float64 autograd + scipy's L-BFGS-B) the tolerances are those of tests/test_gpu_gp_fit.py.

The four states: n = 150 points in d = 12 whose coordinate scales fall off at different rates, so that the weighted PCA keeps
k = (11, 11, 9, 8) components, and the restated scipy fits take 35 / 33 / 29 / 28 evaluations - the runs neither share k nor
finish in the same round."""
import os

import numpy as np
import pytest
import torch

import pcabo_oracle as O
from pcabo.bbob import BBOBProblem
from test_gp_fit_cpu import RestatedFit
from test_gpu_gp_fit import GRAD_TOL, LOSS_TOL, THETAS

pytestmark = pytest.mark.gpu

B, N, D = 4, 150, 12
LO = (1.0, 0.5, 0.2, 0.05)
FIT_KEYS = ("iterations", "evaluations", "warnflag", "task")


def _state(b):
    rng = np.random.default_rng(21 + b)
    X = rng.uniform(-5, 5, (N, D)) * np.linspace(1, LO[b], D)
    y = np.sin(0.7 * X[:, 0]) * 40 + (X ** 2).sum(1) + rng.normal(size=N)
    noise = rng.normal(0, 1e-8, X.shape)
    return X, y, noise


@pytest.fixture(scope="module")
def data():
    torch.set_num_threads(8)
    X, y, noise = (np.stack(a) for a in zip(*[_state(b) for b in range(B)]))
    ranks = np.argsort(np.argsort(y, axis=1), axis=1).astype(np.int64) + 1
    return X, y, noise, ranks


def _pca_batch(native, data, order=range(B)):
    """A batch conditioned (begin) on the states `order`, its wPCA results collected."""
    X, y, noise, ranks = data
    order = list(order)
    bt = native.Batch(len(order), max_n=N, max_d=D, max_q=512)
    bt.wpca_gp_condition_begin(X[order], ranks[order], noise[order], y[order])
    return bt, bt.wpca_results()


def _alone(native, data, b):
    """A stand-alone context holding state b's reduced points (its own weighted PCA, as PCA_BO(fit_gp=True) runs it)."""
    X, y, noise, ranks = data
    c = native.Context(max_n=N, max_d=D, max_q=512)
    res = c.wpca(X[b], ranks=ranks[b], noise=noise[b])
    return c, res


def _same_fit(a, b):
    return (a["theta"].tobytes() == b["theta"].tobytes() and a["loss"] == b["loss"]
            and all(a[key] == b[key] for key in FIT_KEYS))


def test_batch_gp_mll_equals_the_single_context_bit_for_bit(native, data, capsys):
    bt, res = _pca_batch(native, data)
    ks = [r["k"] for r in res]
    assert len(set(ks)) >= 2, ks                      # the runs of the batch differ in k (k_dev is read per run)
    worst_l, worst_g = 0.0, np.zeros(3)
    try:
        for shift in range(len(THETAS)):
            thetas = np.array([THETAS[(b + shift) % len(THETAS)] for b in range(B)])       # another theta per run, the bound included
            out = bt.gp_mll(thetas)
            for b in range(B):
                assert out[b]["status"] == 0
                c, r1 = _alone(native, data, b)
                try:
                    assert r1["k"] == ks[b]
                    one = c.gp_mll(data[1][b], thetas[b])
                finally:
                    c.close()
                assert out[b]["loss"] == one["loss"], (shift, b, out[b]["loss"], one["loss"])
                assert np.array_equal(out[b]["grad"], one["grad"]), (shift, b, out[b]["grad"], one["grad"])
                rf = RestatedFit(r1["Z"], data[1][b])
                lv, lg = rf.value_and_grad(tuple(thetas[b]))
                el = abs(out[b]["loss"] - lv) / max(abs(lv), 1e-2)
                eg = np.abs(out[b]["grad"] - lg) / np.maximum(np.abs(lg), 1e-3 * rf.term_scales(tuple(thetas[b])))
                worst_l, worst_g = max(worst_l, el), np.maximum(worst_g, eg)
                assert el <= LOSS_TOL, (shift, b, out[b]["loss"], lv)
                assert (eg <= GRAD_TOL).all(), (shift, b, out[b]["grad"], lg)
    finally:
        bt.close()
    with capsys.disabled():
        print(f"\n  k = {ks}; Batch.gp_mll vs restatement, worst relative error: loss {worst_l:.2e}, gradient (noise, mean, rho) "
              + " ".join(f"{v:.2e}" for v in worst_g))


def _check_members_against(native, bt, fits, singles, best):
    """After Batch.gp_fit: every member's GP state and acquisition equal the stand-alone context's (fitted the same way)."""
    for b, (c, Z, y) in enumerate(singles):
        stb, st1 = bt.ctx[b].gp_state(), c.gp_state()
        for key in ("L", "R", "alpha"):
            assert np.array_equal(stb[key], st1[key]), (b, key)
        box = bt.ctx[b].acq_bounds()
        assert np.array_equal(box, c.acq_bounds())
        Xq = np.random.default_rng(7 + b).uniform(box[0], box[1], size=(64, Z.shape[1]))
        vb, gb = bt.ctx[b].acq_eval(Xq, best[b], False, native.ACQ_LOG_EI)
        v1, g1 = c.acq_eval(Xq, best[b], False, native.ACQ_LOG_EI)
        assert np.array_equal(vb, v1) and np.array_equal(gb, g1), b
        yield b, Xq, vb, gb


def test_batch_gp_fit_equals_the_single_fits_bit_for_bit(native, data, capsys):
    X, y, noise, ranks = data
    bt, res = _pca_batch(native, data)
    singles = []
    rows = []
    try:
        fits = bt.gp_fit()
        one = []
        for b in range(B):
            c, r1 = _alone(native, data, b)
            singles.append((c, r1["Z"], y[b]))
            one.append(c.gp_fit(y[b]))
            assert fits[b]["status"] == 0
            assert _same_fit(fits[b], one[b]), (b, fits[b], one[b])
        evals = [f["evaluations"] for f in fits]
        assert len(set(evals)) >= 2, evals                # the runs do not all finish in one round: finished ones rest
        assert bt.fit_rounds >= max(evals)
        best = [float(y[b].min()) for b in range(B)]
        for b, Xq, vb, gb in _check_members_against(native, bt, fits, singles, best):
            Z = singles[b][1]
            r = fits[b]
            gp = O.ExactGP(Z, y[b], None, lengthscale=r["lengthscale"], noise=r["noise"])
            gp.y_mean = gp.y_mean + gp.y_std * r["mean_constant"]      # the constant mean: m' = m + s c, y_s - c
            gp.y_s = gp.y_s - r["mean_constant"]
            ov, og = O.Acquisition(gp, best[b], False).value_and_grad(Xq)
            assert (np.abs(vb - ov) / np.maximum(1.0, np.abs(ov))).max() < 1e-8, b
            assert np.abs(gb - og).max() < 1e-7 * max(1.0, np.abs(og).max()), b
            ref = RestatedFit(Z, y[b]).fit()
            rel = np.abs(r["theta"] - ref.x) / np.maximum(np.abs(ref.x), 1e-2)
            rows.append((b, r["theta"], ref.x, rel, r["iterations"], r["evaluations"], ref.nit, ref.nfev))
            assert r["warnflag"] == 0, (b, r)
            assert (rel <= 1e-3).all(), (b, r["theta"], ref.x)
        # the batched scoring after the fit: the same values as the single context's (values only) at the fitted model
        boxes = bt.acq_bounds()
        raw = [boxes[b][0] + (boxes[b][1] - boxes[b][0]) * np.random.default_rng(40 + b).uniform(size=(512, res[b]["k"]))
               for b in range(B)]
        vals, status = bt.gp_wait_eval(raw, best)
        assert not status.any()
        for b in range(B):
            assert np.array_equal(vals[b], singles[b][0].acq_eval(raw[b], best[b], False, native.ACQ_LOG_EI, grad=False)), b
        # ... and one optimise call on every run's own model
        ics = [raw[b][:10] for b in range(B)]
        outs, status = bt.optimize_acqf(ics, boxes, best)
        assert not status.any()
        for b in range(B):
            c = singles[b][0]
            c.set_option(native.OPT_GROUP_ACQ, 1)
            cand, v, info, failed = c.optimize_acqf(ics[b], boxes[b], best[b])
            assert np.array_equal(cand, outs[b][0]) and np.array_equal(v, outs[b][1]) and np.array_equal(info, outs[b][2]), b
    finally:
        bt.close()
        for c, _, _ in singles:
            c.close()
    with capsys.disabled():
        print()
        for b, th, rx, rel, it, ev, rit, rev in rows:
            print(f"  run {b}: device theta {np.array2string(th, precision=8)} ({it} it / {ev} ev), restated "
                  f"{np.array2string(rx, precision=8)} ({rit} it / {rev} ev), worst relative difference {rel.max():.1e}")
        print(f"  lock-step rounds {bt.fit_rounds}")


def test_vanilla_style_batch_gp_fit_equals_the_single_fits(native, data):
    """pcabo_batch_gp_condition_begin with identity Normalize bounds (BatchedVanillaBO): the fit works on the raw points."""
    X, y, _, _ = data
    ident = np.vstack([np.zeros(D), np.ones(D)])
    Zs = X / 10.0 + 0.5                                   # the raw points in the unit box
    bt = native.Batch(B, max_n=N, max_d=D, max_q=512)
    singles = []
    try:
        bt.gp_condition_begin(Zs, y, norm_bounds=ident)
        fits = bt.gp_fit()
        for b in range(B):
            c = native.Context(max_n=N, max_d=D, max_q=512)
            singles.append((c, Zs[b], y[b]))
            one = c.gp_fit(y[b], Z=Zs[b], norm_bounds=ident)
            assert fits[b]["status"] == 0
            assert _same_fit(fits[b], one), (b, fits[b], one)
        best = [float(y[b].min()) for b in range(B)]
        assert len(list(_check_members_against(native, bt, fits, singles, best))) == B
    finally:
        bt.close()
        for c, _, _ in singles:
            c.close()


def test_two_fits_of_one_batch_state_and_a_larger_batch_are_bit_identical(native, data):
    bt, _ = _pca_batch(native, data)
    try:
        first, second = bt.gp_fit(), bt.gp_fit()
    finally:
        bt.close()
    order = [0, 1, 2, 3, 3, 2, 1, 0]
    big, _ = _pca_batch(native, data, order)
    try:
        wide = big.gp_fit()
    finally:
        big.close()
    for b in range(B):
        assert _same_fit(first[b], second[b]), b
    for j, b in enumerate(order):
        assert _same_fit(first[b], wide[j]), (j, b)


def test_parked_runs_do_not_fit_and_rbf_is_refused(native, data):
    bt, _ = _pca_batch(native, data)
    try:
        ref = bt.gp_fit()
        bt.set_active([True, False, True, True])
        fits = bt.gp_fit()
        assert fits[1] == {"status": -1}
        for b in (0, 2, 3):
            assert _same_fit(fits[b], ref[b]), b
    finally:
        bt.close()
    X, y, noise, ranks = data
    bt = native.Batch(B, max_n=N, max_d=D, max_q=512)
    try:
        bt.wpca_gp_condition_begin(X, ranks, noise, y, kernel=native.KERNEL_RBF)
        bt.wpca_results()
        with pytest.raises(native.PcaboError) as e:
            bt.gp_fit()
        assert e.value.code == -1
    finally:
        bt.close()


# ---- whole runs --------------------------------------------------------------------------------------------------------
def _single_pca(fid, inst, dim, budget, n_doe, seed, acq_kernel):
    from Algorithms import PCA_BO
    opt = PCA_BO(budget=budget, n_DoE=n_doe, random_seed=seed, maximization=False, acq_kernel=acq_kernel, fit_gp=True)
    opt(BBOBProblem(fid, inst, dim))
    return opt


@pytest.mark.parametrize("mode", ["group", "latency"])
@pytest.mark.parametrize("dim,budget,n_doe,runs", [(10, 70, 30, 5), (40, 200, 120, 3)])
def test_batched_runs_with_fit_gp_equal_single_runs_bit_for_bit(native, dim, budget, n_doe, runs, mode):
    from pcabo.batchrun import BatchedPCABO
    torch.set_num_threads(4)
    insts = list(range(runs))
    seeds = [15000 + 10 * dim + i for i in insts]
    r = BatchedPCABO([BBOBProblem(15, i, dim) for i in insts], seeds, budget, n_doe, acq_kernel=mode, fit_gp=True)
    r.run()
    assert r.timing["fit"] > 0.0
    for b, i in enumerate(insts):
        opt = _single_pca(15, i, dim, budget, n_doe, seeds[b], mode)
        assert np.array_equal(np.vstack(r.x_evals[b]), np.vstack(opt.x_evals)), (dim, b)
        assert np.array_equal(np.array(r.f_evals[b]), np.array(opt.f_evals)), (dim, b)
        assert r.current_best[b] == opt.current_best and r.current_best_index[b] == opt.current_best_index
        assert r.gp_hyperparameters[b]["theta"].tobytes() == opt.gp_hyperparameters["theta"].tobytes(), (dim, b)


def test_batched_vanilla_runs_with_fit_gp_equal_single_runs_bit_for_bit(native):
    from Algorithms import Vanilla_BO
    from pcabo.batchrun import BatchedVanillaBO
    torch.set_num_threads(4)
    fid, dim, budget, n_doe, runs = 15, 10, 70, 30, 4
    insts = list(range(runs))
    seeds = [1000 * fid + 10 * dim + i for i in insts]
    r = BatchedVanillaBO([BBOBProblem(fid, i, dim) for i in insts], seeds, budget, n_doe, acq_kernel="latency", fit_gp=True)
    r.run()
    assert r.timing["fit"] > 0.0
    for b, i in enumerate(insts):
        opt = Vanilla_BO(budget=budget, n_DoE=n_doe, random_seed=seeds[b], maximization=False, fit_gp=True)
        opt(BBOBProblem(fid, i, dim))
        assert np.array_equal(np.vstack(r.x_evals[b]), np.vstack(opt.x_evals)), b
        assert np.array_equal(np.array(r.f_evals[b]), np.array(opt.f_evals)), b
        assert r.current_best[b] == opt.current_best and r.current_best_index[b] == opt.current_best_index
        assert r.gp_hyperparameters[b]["theta"].tobytes() == opt.gp_hyperparameters["theta"].tobytes(), b


def test_device_stepping_equals_its_twin_with_fit_gp(native):
    from pcabo.batchrun import BatchedPCABO, device_mode_covers
    dim, budget, n_doe, runs = 10, 70, 30, 5
    assert device_mode_covers(dim, budget)
    insts = list(range(runs))
    seeds = [15000 + 10 * dim + i for i in insts]
    out = {}
    for mode in ("device", "device-twin"):
        r = BatchedPCABO([BBOBProblem(15, i, dim) for i in insts], seeds, budget, n_doe, acq_kernel=mode, fit_gp=True)
        r.run()
        assert all(f is None for f in r.failed)
        out[mode] = r
    for b in range(runs):
        assert np.array_equal(np.vstack(out["device"].x_evals[b]), np.vstack(out["device-twin"].x_evals[b])), b
        assert np.array_equal(np.array(out["device"].f_evals[b]), np.array(out["device-twin"].f_evals[b])), b
        assert out["device"].gp_hyperparameters[b]["theta"].tobytes() == out["device-twin"].gp_hyperparameters[b]["theta"].tobytes()


def test_experiment_runner_batched_fit_gp_writes_the_same_files(native, tmp_path):
    from Algorithms import ExperimentRunner
    outs = []
    for batched in (0, 4):
        root = tmp_path / f"b{batched}"
        kw = dict(batched=4, batched_fit_gp=True, batch_acq_kernel="latency") if batched else dict(batched=0, fit_gp=True)
        er = ExperimentRunner(algorithms=["pca"], dimensions=[5], problem_ids=[15, 20], num_runs=3, budget_factor=5,
                              doe_factor=2.0, root_dir=str(root), experiment_name="experiment", progress=False, **kw)
        er.run_experiment()
        assert len(er.results) == 6
        outs.append((root, sorted((r["problem_id"], r["instance"], r["best"]) for r in er.results), er.results))
    assert outs[0][1] == outs[1][1]
    assert all(r["SingleTaskGP"] > 0.0 for r in outs[1][2])          # the fit's share of a run's time
    for fid, name in ((15, "RastriginRotated"), (20, "Schwefel")):
        rel = os.path.join("pca-experiment", f"data_f{fid}_{name}", f"IOHprofiler_f{fid}_DIM5.dat")
        a, b = open(os.path.join(outs[0][0], rel)).read(), open(os.path.join(outs[1][0], rel)).read()
        assert a == b
    meta = open(os.path.join(outs[1][0], "pca-experiment", "IOHprofiler_f15_RastriginRotated.json")).read()
    assert '"gp_fit": "map"' in meta


def test_a_batch_without_fit_gp_is_unchanged(native):
    """fit_gp=False: no fit call, no hyperparameter block read - the run of tests/test_gpu_batch.py, the `fit` clock at zero."""
    from Algorithms import PCA_BO
    from pcabo.batchrun import BatchedPCABO
    dim, budget, n_doe = 10, 70, 30
    insts = [0, 1]
    seeds = [15000 + 10 * dim + i for i in insts]
    r = BatchedPCABO([BBOBProblem(15, i, dim) for i in insts], seeds, budget, n_doe, acq_kernel="group")
    r.run()
    assert r.timing["fit"] == 0.0 and r.gp_hyperparameters == [None, None]
    for b, i in enumerate(insts):
        opt = PCA_BO(budget=budget, n_DoE=n_doe, random_seed=seeds[b], maximization=False, acq_kernel="group")
        opt(BBOBProblem(15, i, dim))
        assert np.array_equal(np.vstack(r.x_evals[b]), np.vstack(opt.x_evals)), b
        assert np.array_equal(np.array(r.f_evals[b]), np.array(opt.f_evals)), b
