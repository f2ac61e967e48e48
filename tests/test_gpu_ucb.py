"""The upper-confidence-bound acquisition on the device (PCABO_ACQ_UCB: the third branch of `acq_scalar_chain` in
acq_math.h, which kernels_acq.hip and `lb_eval` in kernels_lbfgsb.hip share; kappa = sqrt(beta) travels in the `best_f` slot):

  * value and gradient of every evaluation path against the reference UCB on the oracle's exact GP (tests/ucb_reference.py);
  * bad kappa / unknown acquisition codes are argument errors that leave the context usable;
  * a run inside a batch equals the same run alone, the device-resident L-BFGS-B equals its host-stepped twin, bit for bit;
  * a free PCA_BO run replayed iteration by iteration from the oracle's public functions.
The tolerances of the first are measured ones; tests/test_gpu_ucb_edges.py judges the same paths in derived fp64 error units.
"""
import numpy as np
import pytest
import torch

import pcabo_oracle as O
from pcabo.bbob import BBOBProblem
from test_gpu_late_phase import _rel
from ucb_reference import UCBReference, kappa_of

pytestmark = pytest.mark.gpu

# state -> (n, k, scale of y, kernel): the smallest shapes that reach each code form
STATES = {
    "A": (9, 1, 1.0, "matern52"),          # k_acq_fast, NP = 64, one component
    "B": (70, 6, 1.0, "matern52"),         # k_acq_fast, NP = 128, 16-row slabs
    "B-rbf": (70, 6, 1.0, "rbf"),
    "C": (449, 10, 1.0, "matern52"),       # k_acq_fast, NP = 512, 32-row slabs; lb_eval with 2 row parts
    "D": (50, 41, 1.0, "matern52"),        # k_acq_fused (k > 40); host-paced paths only
    "E": (30, 3, 1e-7, "matern52"),        # every query's variance under gpytorch's 1e-10 floor
}
COMBOS = [(False, 0.25), (False, 2.0), (True, 0.25), (True, 2.0)]      # (maximize, beta)

# Worst error per evaluation path over all states and combinations, MEASURED on an MI355X against the reference (value:
# |dv| / max(1, |v|); gradient: _rel) - see the table in EXPERIMENTS.md; asserted: 10 x measured, and never above what the
# project asserts for log-EI on the same kernels (value 1e-8, gradient 1e-6).
#   path          what runs                                                     measured value / gradient
MEASURED = {
    "finish32":  (1.54e-13, 1.84e-13),   # q = 32: per-query kernels, in-launch finish                          (worst: state C)
    "combine40": (1.54e-13, 1.84e-13),   # q = 40: partial records + k_acq_combine, with gradients              (C)
    "gemm512":   (3.29e-13, None),       # q = 512 through gp_wait_eval: GEMM scoring + k_acq_combine, values   (B-rbf)
    "group32":   (1.64e-13, 1.93e-13),   # PCABO_OPT_GROUP_ACQ = 1, q = 32: k_acq_group                         (C)
    "group40":   (1.54e-13, 1.84e-13),   # the same context, q = 40                                             (C)
    "group512":  (3.29e-13, None),       # the same context, q = 512 through gp_wait_eval                       (B-rbf)
    "batch512":  (3.29e-13, None),       # Batch.gp_wait_eval: the batched scoring launch                       (B-rbf)
    "device32":  (1.77e-13, 1.87e-13),   # Batch(device_lbfgsb=1).device_acq_eval: lb_eval of k_lbfgsb_group    (C)
}
CEILING = (1e-8, 1e-6)
FAMILIES_AGREE = 1e-10                 # the kernel families on the same factor (tests/test_gpu_device_lbfgsb.py)


def _limit(path):
    mv, mg = MEASURED[path]
    return min(10 * mv, CEILING[0]), (None if mg is None else min(10 * mg, CEILING[1]))


def _make(name):
    n, k, yscale, kernel = STATES[name]
    rng = np.random.default_rng(1000 + 10 * n + k)
    Z = rng.normal(size=(n, k))
    y = (rng.normal(size=n) * 30.0 + 200.0) * yscale
    return n, k, kernel, Z, y, rng


def _verr(v, ov):
    return float((np.abs(v - ov) / np.maximum(1.0, np.abs(ov))).max())


@pytest.mark.parametrize("name", list(STATES))
def test_value_and_gradient_against_the_reference_on_every_path(native, name):
    torch.set_num_threads(4)
    n, k, kernel, Z, y, rng = _make(name)
    kcode = native.KERNEL_RBF if kernel == "rbf" else native.KERNEL_MATERN52
    gp = O.ExactGP(Z, y, kernel=kernel)
    ctx = native.Context(max_n=n, max_d=k, max_q=512)
    grp = native.Context(max_n=n, max_d=k, max_q=512)
    grp.set_option(native.OPT_GROUP_ACQ, 1)
    ctx.gp_condition(y, Z=Z, kernel=kcode)
    box = ctx.acq_bounds()
    assert np.abs(box - O.acq_bounds(Z)).max() < 1e-12 * max(1.0, np.abs(box).max())
    X = np.vstack([rng.uniform(box[0], box[1], size=(510, k)), Z[:2]])       # uniform in the search box + two training points
    X[30:32], X[38:40] = Z[:2], Z[:2]                                        # (in every prefix the paths below take)
    on_device = k <= 40                                                       # the device optimiser's limit (state D: host-paced only)
    bt = native.Batch(1, max_n=n, max_d=k, max_q=512, device_lbfgsb=1) if on_device else None
    worst = {}

    def note(path, v, ov, g=None, og=None):
        w = worst.setdefault(path, [0.0, 0.0])
        w[0] = max(w[0], _verr(v, ov))
        if g is not None:
            w[1] = max(w[1], _rel(g, og))

    with torch.no_grad():
        mean = gp.posterior(torch.from_numpy(X))[0].numpy()
    for maximize, beta in COMBOS:
        kappa, ref = kappa_of(beta), UCBReference(gp, beta, maximize)
        ov, og = ref.value_and_grad(X)
        A = native.ACQ_UCB
        v32, g32 = ctx.acq_eval(X[:32], kappa, maximize, A)
        note("finish32", v32, ov[:32], g32, og[:32])
        v40, g40 = ctx.acq_eval(X[:40], kappa, maximize, A)
        note("combine40", v40, ov[:40], g40, og[:40])
        ctx.gp_condition(y, Z=Z, kernel=kcode, wait=False)
        note("gemm512", ctx.gp_wait_eval(X, kappa, maximize, A), ov)
        grp.gp_condition(y, Z=Z, kernel=kcode, wait=False)
        note("group512", grp.gp_wait_eval(X, kappa, maximize, A), ov)
        vg, gg = grp.acq_eval(X[:32], kappa, maximize, A)
        note("group32", vg, ov[:32], gg, og[:32])
        vg40, gg40 = grp.acq_eval(X[:40], kappa, maximize, A)
        note("group40", vg40, ov[:40], gg40, og[:40])
        between = [_verr(vg, v32), _rel(gg, g32), _verr(v40[:32], v32), _rel(g40[:32], g32)]
        if bt is not None:
            bt.gp_condition_begin(Z[None], y[None], kernel=kcode)
            vb, st = bt.gp_wait_eval([X], [kappa], maximize, A)
            assert not st.any()
            note("batch512", vb[0], ov)
            vd, gd = bt.device_acq_eval([X[:32]], [kappa], maximize, A)
            note("device32", vd[0], ov[:32], gd[0], og[:32])
            between += [_verr(vd[0], v32), _rel(gd[0], g32)]
        assert max(between) < FAMILIES_AGREE, (name, maximize, beta, between)
        if name == "E":
            # sigma is the floor's sqrt(1e-10) at every query: the kappa term is a constant and its gradient exactly zero
            sgn = 1.0 if maximize else -1.0
            for v, m in ((v32, mean[:32]), (vg, mean[:32]), (v40, mean[:40])) + (((vd[0], mean[:32]),) if bt is not None else ()):
                assert np.abs((v - sgn * m) - kappa * 1e-5).max() <= 1e-12 * kappa * 1e-5, (maximize, beta)
            v0, g0 = ctx.acq_eval(X[:32], 0.0, maximize, A)                   # kappa = 0: the mean alone
            assert np.array_equal(g0, g32)                                    # ... has the same gradient, bit for bit
            scale = float(np.abs(og[:32]).max())                              # (tiny here: judged relative to itself)
            assert np.abs(g32 - og[:32]).max() <= CEILING[1] * scale and np.abs(gd[0] - og[:32]).max() <= CEILING[1] * scale
    print("[UCB vs reference, state %s (n=%d k=%d %s)] " % (name, n, k, kernel)
          + "; ".join("%s value %.2e%s" % (p, w[0], "" if MEASURED[p][1] is None else " gradient %.2e" % w[1])
                      for p, w in worst.items()))
    for path, w in worst.items():
        lv, lg = _limit(path)
        assert w[0] <= lv and (lg is None or w[1] <= lg), (name, path, w, (lv, lg))
    ctx.close()
    grp.close()
    if bt is not None:
        bt.close()


@pytest.mark.parametrize("n,k", [(50, 33), (50, 40), (50, 64), (100, 65), (100, 128)])
def test_group_kernel_with_fewer_points_than_twice_the_components(native, n, k):
    """State D met this on the way: k_acq_group stages its gradient parts ([10][k] doubles) in the LDS region of its kernel
    vectors ([5][NP]), which is the smaller of the two where NP < 2 k - the parts ran over into a wave's reduction tile and
    the gradients of full groups came out wrong (values were right), for every acquisition.  The region now has the larger
    size.  Log-EI and UCB, group kernel against the per-query kernels on the same factor."""
    rng = np.random.default_rng(7000 + 10 * n + k)
    Z = rng.normal(size=(n, k))
    y = rng.normal(size=n) * 30.0 + 200.0
    ctx = native.Context(max_n=n, max_d=k, max_q=64)
    grp = native.Context(max_n=n, max_d=k, max_q=64)
    grp.set_option(native.OPT_GROUP_ACQ, 1)
    ctx.gp_condition(y, Z=Z)
    grp.gp_condition(y, Z=Z)
    box = ctx.acq_bounds()
    X = rng.uniform(box[0], box[1], size=(13, k)) * 0.5 + 0.5 * Z[:13]
    for scalar, code in ((float(y.min()), native.ACQ_LOG_EI), (kappa_of(2.0), native.ACQ_UCB)):
        v, g = ctx.acq_eval(X, scalar, False, code)
        vg, gg = grp.acq_eval(X, scalar, False, code)
        assert _verr(vg, v) < FAMILIES_AGREE and _rel(gg, g) < FAMILIES_AGREE, (n, k, code, _verr(vg, v), _rel(gg, g))
    ctx.close()
    grp.close()


def test_bad_kappa_and_unknown_codes_are_argument_errors(native):
    n, k, kernel, Z, y, rng = _make("B")
    ctx = native.Context(max_n=n, max_d=k, max_q=64)
    ctx.gp_condition(y, Z=Z)
    box = ctx.acq_bounds()
    X = rng.uniform(box[0], box[1], size=(10, k))
    kappa = kappa_of(2.0)
    good_v, good_g = ctx.acq_eval(X, kappa, False, native.ACQ_UCB)
    bad = [(-1.0, native.ACQ_UCB), (float("nan"), native.ACQ_UCB), (float("inf"), native.ACQ_UCB), (0.0, 3), (kappa, -1)]
    for scalar, code in bad:
        for call in (lambda: ctx.acq_eval(X, scalar, False, code),
                     lambda: ctx.optimize_acqf(X, box, scalar, False, code)):
            with pytest.raises(native.PcaboError) as e:
                call()
            assert e.value.code == -1, (scalar, code)
        v, g = ctx.acq_eval(X, kappa, False, native.ACQ_UCB)                  # the context is as usable as before
        assert np.array_equal(v, good_v) and np.array_equal(g, good_g)
    ctx.gp_condition(y, Z=Z, wait=False)
    with pytest.raises(native.PcaboError) as e:
        ctx.gp_wait_eval(X, -1.0, False, native.ACQ_UCB)
    assert e.value.code == -1
    assert np.array_equal(ctx.gp_wait_eval(X, kappa, False, native.ACQ_UCB), good_v)
    cand, vals, info, failed = ctx.optimize_acqf(X, box, kappa, False, native.ACQ_UCB)
    assert not failed and np.isfinite(cand).all()
    assert vals[:5].sum() >= good_v[:5].sum() and vals[5:].sum() >= good_v[5:].sum()      # a joint group ends no lower than it began
    ctx.close()
    # a batch: the scalars of the active runs are checked, a parked run's slot is not
    bt = native.Batch(2, max_n=n, max_d=k, max_q=64, device_lbfgsb=1)
    bt.gp_condition_begin(np.stack([Z, Z]), np.stack([y, y]))
    for scalars, code in (([kappa, -1.0], native.ACQ_UCB), ([float("nan"), kappa], native.ACQ_UCB), ([kappa, kappa], 3)):
        with pytest.raises(native.PcaboError) as e:
            bt.gp_wait_eval([X, X], scalars, False, code)
        assert e.value.code == -1
    vb, st = bt.gp_wait_eval([X, X], [kappa, kappa], False, native.ACQ_UCB)
    assert not st.any() and np.array_equal(vb[0], vb[1])
    for call in (lambda s: bt.device_acq_eval([X, X], s, False, native.ACQ_UCB),
                 lambda s: bt.optimize_acqf([X, X], [box, box], s, False, native.ACQ_UCB)):
        with pytest.raises(native.PcaboError) as e:
            call([kappa, float("nan")])
        assert e.value.code == -1
    vd, gd = bt.device_acq_eval([X, X], [kappa, kappa], False, native.ACQ_UCB)
    assert _verr(vd[0], good_v) < FAMILIES_AGREE and np.array_equal(vd[0], vd[1])
    bt.set_active([1, 0])
    outs, status = bt.optimize_acqf([X, X], [box, box], [kappa, float("nan")], False, native.ACQ_UCB)
    assert status[0] == 0 and status[1] == -1 and np.isfinite(outs[0][0]).all()
    bt.close()


UCB = dict(acquisition_function="UCB", ucb_beta=2.0)


@pytest.mark.parametrize("acq_kernel", ["latency", "group"])
def test_batched_ucb_runs_equal_single_runs_bit_for_bit(native, acq_kernel):
    from Algorithms import PCA_BO
    from pcabo.batchrun import BatchedPCABO
    torch.set_num_threads(4)
    fid, dim, budget, n_doe, insts = 15, 6, 20, 10, [0, 1, 2]
    seeds = [15000 + 10 * dim + i for i in insts]
    r = BatchedPCABO([BBOBProblem(fid, i, dim) for i in insts], seeds, budget, n_doe, acq_kernel=acq_kernel, **UCB)
    r.run()
    assert r.failed == [None] * 3
    for b, i in enumerate(insts):
        opt = PCA_BO(budget=budget, n_DoE=n_doe, random_seed=seeds[b], maximization=False, acq_kernel=acq_kernel, **UCB)
        opt(BBOBProblem(fid, i, dim))
        assert len(opt.f_evals) == budget
        assert np.array_equal(np.vstack(r.x_evals[b]), np.vstack(opt.x_evals)), (acq_kernel, b)
        assert np.array_equal(np.array(r.f_evals[b]), np.array(opt.f_evals)), (acq_kernel, b)
        assert r.current_best[b] == opt.current_best and r.current_best_index[b] == opt.current_best_index


def test_device_stepping_equals_host_stepping_bit_for_bit_on_ucb(native):
    from test_gpu_device_lbfgsb import _run
    torch.set_num_threads(4)
    fid, dim, budget, n_doe, B = 15, 10, 50, 30, 3
    insts = list(range(B))
    keep = lambda b, n: True
    dev = _run(fid, insts, dim, budget, n_doe, "device", record_trace=True, trace_filter=keep, **UCB)
    twin = _run(fid, insts, dim, budget, n_doe, "device-twin", record_trace=True, trace_filter=keep, **UCB)
    assert dev.acq_code == twin.acq_code == native.ACQ_UCB
    assert dev.failed == twin.failed == [None] * B
    for b in range(B):
        assert np.array_equal(np.vstack(dev.x_evals[b]), np.vstack(twin.x_evals[b])), b
        assert np.array_equal(np.array(dev.f_evals[b]), np.array(twin.f_evals[b])), b
    assert len(dev.trace) == len(twin.trace) == B * (budget - n_doe)
    rounds = 0
    for td, tt in zip(dev.trace, twin.trace):
        assert (td["b"], td["n"]) == (tt["b"], tt["n"])
        assert np.array_equal(td["cands"], tt["cands"]) and np.array_equal(td["vals"], tt["vals"]), (td["b"], td["n"])
        assert np.array_equal(td["info"], tt["info"]), (td["b"], td["n"], td["info"], tt["info"])
        rounds += int(np.asarray(td["info"])[:, 1].sum())
    print("[UCB device = twin, f%d d=%d] %d runs x %d iterations, %d L-BFGS-B evaluations compared" % (fid, dim, B, budget - n_doe, rounds))


def test_free_ucb_run_replayed_from_the_oracles_public_functions(native):
    from Algorithms import PCA_BO, Vanilla_BO
    torch.set_num_threads(4)
    kw = dict(budget=14, n_DoE=8, record_trace=True, **UCB)
    opt = PCA_BO(**kw)
    opt(BBOBProblem(15, 2, 6))
    assert opt.acquisition_function_name == "upper_confidence_bound"
    assert len(opt.f_evals) == 14 and len(opt.trace) == 6                     # the run reaches its budget
    X_all, f_all = np.vstack(opt.x_evals), np.array(opt.f_evals, dtype=np.float64)
    for tr in opt.trace:
        n = tr["n"]
        X, f = X_all[:n], f_all[:n]
        np.random.set_state(tr["numpy_state"])
        torch.set_rng_state(tr["torch_state"])
        ranks = O.calculate_ranks(list(f), False)
        noise = np.random.normal(0, 1e-8, size=X.shape)
        wp = O.weighted_pca(X, list(f), False, 0.95, 0, noise=noise, ranks=ranks)
        gp = O.ExactGP(wp.Z, f, O.normalize_bounds(wp.Z))
        trace = O.AcqfTrace()
        O.optimize_acqf(UCBReference(gp, 2.0, False), O.acq_bounds(wp.Z), trace=trace)
        assert wp.k == tr["k"] and trace.retried == bool(tr.get("retried", False))
        err = (float(np.abs(trace.ics - tr["ics"]).max()),
               float((np.abs(trace.vals - tr["vals"]) / np.maximum(1.0, np.abs(trace.vals))).max()),
               float(np.abs(trace.cands - tr["cands"]).max() / max(1.0, np.abs(trace.cands).max())))
        print("[UCB replay n=%d k=%d] initial conditions %.2e, values %.2e, candidates %.2e" % ((n, wp.k) + err))
        assert err[0] < 1e-9 and err[1] < 1e-6 and err[2] < 2e-4
    van = Vanilla_BO(**kw)
    van(BBOBProblem(15, 2, 6))
    assert len(van.f_evals) == 14
    for cls in (PCA_BO, Vanilla_BO):      # without ucb_beta: the reference's TypeError after the DoE (test_gpu_parity.py is the authority)
        plain = cls(budget=14, n_DoE=8, acquisition_function="UCB")
        with pytest.raises(TypeError):
            plain(BBOBProblem(15, 2, 6))
        assert plain.number_of_function_evaluations == 8
