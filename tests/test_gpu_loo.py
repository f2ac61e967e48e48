"""Leave-one-out predictions on the MI355X (pcabo_gp_loo / pcabo_batch_gp_loo: k_loo; Context.gp_loo, Batch.gp_loo, PCA_BO.loo,
Vanilla_BO.loo) against tests/loo_reference.py.

Two comparisons, kept apart:
  kernel arithmetic  gp_loo() against closed_form (extended precision) of the DEVICE's own R, alpha and (m', s) as gp_state()
                     hands them out, in the error units of loo_reference.units: 16 units for all four vectors, and lpd_sum bit-equal
                     to the index-order fp64 sum of the returned lpd.  Shapes: n in {2, 3, 63, 64, 65, 129, 257} x k in {1, 5, 33}
                     (a partial block, one block, one block and one row, several blocks) and the latest state of
                     tests/golden/late_state_d40.npz (n = 420: the file holds the states 320, 384 and 420, none of 449 points);
                     the hyperparameter sets of gp_reference at n = 65 and 129.
  end to end         gp_loo() against brute_force (a refit of n - 1 points per point in extended precision): the mean in LOO standard
                     deviations, the variance relative, z and lpd absolute.  The yardstick of a case is the distance between the
                     plain fp64 numpy restatement of the whole chain (loo_reference.restate_chain) and the same brute force, largest
                     over the points, floored at 64 * 2^-53; the device may be 32 x that away: its blocked Cholesky and explicit
                     inverse have other constants of the same order than LAPACK's (tests/test_gpu_gp_edges.py shows that for the
                     factors themselves).  The tests print device / yardstick per case; EXPERIMENTS.md keeps the table.
"""
import os

import numpy as np
import pytest

import loo_reference as LR
import pcabo_oracle as O
from ard_reference import ard_state
from gp_reference import HYPERS, make_case
from pcabo.bbob import BBOBProblem
from test_gpu_batch_ard import KS9, SEEDS9, _alone, _batch, batch_data

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "late_state_d40.npz")
GRID = [(n, k, "default") for n in (2, 3, 63, 64, 65, 129, 257) for k in (1, 5, 33)]
GRID += [(n, 5, h) for n in (65, 129) for h in HYPERS[1:]]
FLOOR, ALLOWED = 64.0 * 2.0 ** -53, 32.0
E2E = [("lhs", 65, 3, "default"), ("cluster", 65, 3, "default"), ("lhs", 130, 9, "short"), ("lhs", 64, 5, "rbf")]
ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=449, max_d=64, max_q=64)
    yield c
    c.close()


def _condition(native, ctx, case):
    ctx.gp_condition(case.y, Z=case.Z, norm_bounds=case.norm_bounds, lengthscale=case.lengthscale, noise=case.noise,
                     kernel=native.KERNEL_RBF if case.kernel == "rbf" else native.KERNEL_MATERN52)


def _arithmetic(ctx, y, what):
    """gp_loo() of the context's state in units of the closed form on its own gp_state(); the sum's bits."""
    out, st = ctx.gp_loo(), ctx.gp_state()
    n = len(y)
    assert all(out[key].shape == (n,) for key in LR.KEYS)
    cf = LR.closed_form(st["R"], st["alpha"], y, (st["y_mean"], st["y_std"]))
    ratios = LR.unit_ratios(out, cf)
    print("  %s: units %s" % (what, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= LR.LIMIT, (what, ratios)
    total = 0.0
    for v in out["lpd"]:
        total += float(v)
    assert np.float64(total).tobytes() == np.float64(out["lpd_sum"]).tobytes(), what
    assert (out["variance"] > 0.0).all()
    return out, st


def _end_to_end(out, case, what):
    """Distances of the device and of the fp64 restatement from the brute force; the device within ALLOWED x the yardstick."""
    bf = LR.brute_force(case)
    dev, ref = LR.distances(out, bf), LR.distances(LR.restate_chain(case), bf)
    ratios = {key: dev[key] / max(ref[key], FLOOR) for key in LR.KEYS}
    print("  %s: device / yardstick %s" % (what, " ".join("%s %.2e / %.2e = %.2f" % (k, dev[k], max(ref[k], FLOOR), ratios[k])
                                                             for k in LR.KEYS)))
    assert max(ratios.values()) <= ALLOWED, (what, dev, ref)


# ---- kernel arithmetic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,hyper", GRID, ids=lambda v: str(v))
def test_kernel_arithmetic_on_the_device_state(native, ctx, n, k, hyper):
    case = make_case("lhs", n, k, hyper)
    _condition(native, ctx, case)
    _arithmetic(ctx, case.y, case.id)


def test_kernel_arithmetic_on_the_late_state(native, ctx):
    data = np.load(GOLDEN)
    n = int(data["ns"][-1])
    X, f = data["X"][:n], np.asarray(data["f"][:n], dtype=np.float64)
    assert X.shape[0] == n == 420
    res = O.weighted_pca(X, f, False, 0.95, 0, noise=np.random.default_rng(n).normal(0.0, 1e-8, size=X.shape))
    ctx.gp_condition(f, Z=np.ascontiguousarray(res.Z))
    _arithmetic(ctx, f, "late state n = %d, k = %d" % (n, res.Z.shape[1]))


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen,n,k,hyper", E2E, ids=lambda v: str(v))
def test_end_to_end_against_the_refit(native, ctx, gen, n, k, hyper):
    case = make_case(gen, n, k, hyper)
    _condition(native, ctx, case)
    out, _ = _arithmetic(ctx, case.y, case.id)
    _end_to_end(out, case, case.id)


# ---- fitted models -----------------------------------------------------------------------------------------------------------
def _model_case(Z, y, hp, st, ard):
    """The reference's case of a fitted state: the scalar fit's lengthscale with the data's own Normalize range, or the FOLDED
    bounds of an ARD fit as gp_state() reports them with lengthscale 1."""
    case = make_case("lhs", Z.shape[0], Z.shape[1])
    case.Z, case.y, case.noise, case.mean_c = np.ascontiguousarray(Z), y, hp["noise"], hp["mean_constant"]
    case.lengthscale, case.norm_bounds = (1.0, st["norm_bounds"]) if ard else (hp["lengthscale"], None)
    return case


@pytest.mark.parametrize("model", ["gp_fit", "gp_fit_ard", "gp_mll"])
def test_fitted_models(native, ctx, model):
    Z, y = ard_state(2, 65, 3)
    if model == "gp_fit":
        hp = ctx.gp_fit(y, Z=Z)
    elif model == "gp_fit_ard":
        hp = ctx.gp_fit_ard(y, Z=Z)
    else:
        hp = ctx.gp_mll(y, theta=(0.02, 0.3, 0.5), Z=Z)
        assert hp["mean_constant"] == 0.3
    out, st = _arithmetic(ctx, y, model)
    c = hp["mean_constant"]
    assert c != 0.0
    want = y.mean() + y.std(ddof=1) * c                          # the mean constant shows in ystats[0]: m' = m + s c, two n-term
    tol = (len(y) + 4) * 2.0 ** -52 * (np.abs(y).mean() + y.std(ddof=1) * abs(c))      # sums and a few operations on either side
    assert abs(st["y_mean"] - want) <= tol and abs(st["y_mean"] - y.mean()) > 0.1 * y.std(ddof=1) * abs(c), (st["y_mean"], want)
    _end_to_end(out, _model_case(Z, y, hp, st, model == "gp_fit_ard"), model)


# ---- a call leaves no trace ---------------------------------------------------------------------------------------------------
def test_a_call_leaves_no_trace(native, ctx):
    case = make_case("lhs", 129, 5)
    rng = np.random.default_rng(5)
    lo, hi = case.Z.min(0), case.Z.max(0)
    few, many = rng.uniform(lo, hi, size=(5, 5)), rng.uniform(lo, hi, size=(64, 5))
    best = float(case.y.min())

    def sequence(with_loo):
        got = []
        _condition(native, ctx, case)
        loo = lambda: got.append(ctx.gp_loo()) if with_loo else None       # noqa: E731
        loo()
        v, g = ctx.acq_eval(few, best)
        loo()
        s = ctx.acq_eval(many, best, grad=False)
        loo()
        p = ctx.gp_posterior(many, observation_noise=True, covariance=True)
        loo()
        v2, g2 = ctx.acq_eval(few, best)
        return [v, g, s, p["mean"], p["variance"], p["covariance"], v2, g2], got

    plain, _ = sequence(False)
    probed, loos = sequence(True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, probed))
    assert len(loos) == 4
    for other in loos[1:]:                                       # ... and a second call gives the first one's bits
        assert all(np.asarray(other[key]).tobytes() == np.asarray(loos[0][key]).tobytes() for key in loos[0])


def test_outputs_are_host_arrays_in_device_pointer_mode(native, ctx):
    case = make_case("lhs", 65, 5)
    _condition(native, ctx, case)
    host = ctx.gp_loo()
    assert native.LIB.pcabo_set_pointer_mode(ctx._h, native.PTR_DEVICE) == 0
    try:
        dev = ctx.gp_loo()
    finally:
        assert native.LIB.pcabo_set_pointer_mode(ctx._h, native.PTR_HOST) == 0
    assert all(np.asarray(dev[key]).tobytes() == np.asarray(host[key]).tobytes() for key in host)


# ---- a batch: one launch, every run bit for bit what it takes alone ------------------------------------------------------------
SENTINEL = -12345.678


def _raw_batch_loo(native, bt):
    B, n = bt.B, bt.n
    vec = [np.full((B, n), SENTINEL) for _ in range(4)]
    total, status = np.full(B, SENTINEL), np.full(B, 77, dtype=np.int32)
    p = native._ptr
    bt._chk(native.LIB.pcabo_batch_gp_loo(bt._h, p(vec[0]), p(vec[1]), p(vec[2]), p(vec[3]), p(total), p(status)))
    return dict(zip(LR.KEYS, vec), lpd_sum=total), status


def _check_batch(native, bt, singles, parked, what):
    raw, status = _raw_batch_loo(native, bt)
    dicts = bt.gp_loo()
    for b, c in enumerate(singles):
        if b == parked:
            assert status[b] == ERR_ARG and dicts[b] is None
            assert all((raw[key][b] == SENTINEL).all() for key in raw), (what, b)        # its blocks are left as they are
            continue
        one = c.gp_loo()
        assert status[b] == 0
        for key in LR.KEYS:
            assert raw[key][b].tobytes() == one[key].tobytes() == dicts[b][key].tobytes(), (what, b, key)
        assert np.float64(raw["lpd_sum"][b]).tobytes() == np.float64(one["lpd_sum"]).tobytes(), (what, b)
        assert dicts[b]["lpd_sum"] == one["lpd_sum"]


@pytest.mark.parametrize("shape", ["n65-B3-parked", "n130-B3-parked", "n65-B9"])
def test_batch_equals_alone(native, shape):
    n = 130 if shape.startswith("n130") else 65
    ks, seeds = (KS9, SEEDS9) if shape.endswith("B9") else ((5, 3, 1), (12, 13, 14))
    parked = 1 if shape.endswith("parked") else None
    data = batch_data(n, ks, seeds)
    y = data[1]
    B = len(ks)
    bt, res = _batch(native, data, max_q=64)
    singles = []
    try:
        assert [r["k"] for r in res] == list(ks)                 # the runs differ in k
        with pytest.raises(native.PcaboError) as e:              # the conditioning has not been waited for
            bt.gp_loo()
        assert e.value.code == ERR_ARG
        boxes = bt.acq_bounds()
        Xq = [np.random.default_rng(40 + b).uniform(boxes[b][0], boxes[b][1], size=(64, ks[b])) for b in range(B)]
        _, status = bt.gp_wait_eval(Xq, y.min(axis=1))
        assert (status == 0).all()
        if parked is not None:
            bt.set_active([b != parked for b in range(B)])
        for b in range(B):
            singles.append(_alone(native, data, b, max_q=64)[0])
            singles[b].gp_condition(y[b])
        _check_batch(native, bt, singles, parked, "conditioned")
        bt.close()                                               # a fit starts from a conditioning in flight; a fresh batch, so
        bt, res = _batch(native, data, max_q=64)                 # that its weighted PCA is the first one, as the singles' is
        assert [r["k"] for r in res] == list(ks)
        if parked is not None:
            bt.set_active([b != parked for b in range(B)])
        fits = bt.gp_fit()
        for b, c in enumerate(singles):
            if b != parked:
                assert c.gp_fit(y[b])["theta"].tobytes() == fits[b]["theta"].tobytes()
        _check_batch(native, bt, singles, parked, "gp_fit")
        fits = bt.gp_fit_ard()
        for b, c in enumerate(singles):
            if b != parked:
                assert c.gp_fit_ard(y[b])["theta"].tobytes() == fits[b]["theta"].tobytes()
        _check_batch(native, bt, singles, parked, "gp_fit_ard")
    finally:
        for c in singles:
            c.close()
        bt.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refused(native, call):
    with pytest.raises(native.PcaboError) as e:
        call()
    assert e.value.code == ERR_ARG


def test_refusals_leave_the_context_usable(native):
    Z, y = ard_state(11, 40, 3)
    c = native.Context(max_n=64, max_d=3, max_q=32)
    try:
        _refused(native, c.gp_loo)                                                            # never conditioned
        c.gp_condition(y, Z=Z)
        good = c.gp_loo()
        _refused(native, lambda: c._chk(native.LIB.pcabo_gp_loo(c._h, None, None, None, None, None)))      # no output
        assert "NULL" in c._err()
        mean = np.empty(40)                                                                   # any one output will do
        c._chk(native.LIB.pcabo_gp_loo(c._h, native._ptr(mean), None, None, None, None))
        assert mean.tobytes() == good["mean"].tobytes()
        total = native.C.c_double(0.0)                                                        # the sum without its terms
        c._chk(native.LIB.pcabo_gp_loo(c._h, None, None, None, None, native.C.byref(total)))
        assert total.value == good["lpd_sum"]
        c.gp_condition(y, Z=Z, wait=False)
        _refused(native, c.gp_loo)                                                            # between _begin and _end
        c.gp_wait()
        again = c.gp_loo()
        assert all(np.asarray(again[key]).tobytes() == np.asarray(good[key]).tobytes() for key in good)
        Zc = Z.copy()
        Zc[:, 1] = 0.5                                                                        # a Normalize range of 0: K is not finite
        with pytest.raises(native.PcaboError):
            c.gp_condition(y, Z=Zc)
        _refused(native, c.gp_loo)                                                            # the last conditioning left no GP
        c.gp_condition(y, Z=Z)
        again = c.gp_loo()
        assert all(np.asarray(again[key]).tobytes() == np.asarray(good[key]).tobytes() for key in good)
    finally:
        c.close()


def test_batch_refusals(native):
    data = batch_data(40, (3, 1), (13, 14))
    y = data[1]
    bt, _ = _batch(native, data, max_q=64)
    try:
        boxes = bt.acq_bounds()
        Xq = [np.random.default_rng(50 + b).uniform(boxes[b][0], boxes[b][1], size=(64, k)) for b, k in enumerate((3, 1))]
        token = bt.gp_eval_begin(Xq, y.min(axis=1))
        _refused(native, bt.gp_loo)                                                           # a _begin call without its _end
        bt.gp_eval_end(token)
        good = bt.gp_loo()
        assert good[0] is not None and good[1] is not None
        assert native.LIB.pcabo_batch_gp_loo(bt._h, None, None, None, None, None, None) == ERR_ARG     # no output
        assert "NULL" in bt._err()
        again = bt.gp_loo()
        assert all(again[b][key].tobytes() == good[b][key].tobytes() for b in range(2) for key in LR.KEYS)
    finally:
        bt.close()
    fresh = native.Batch(2, max_n=40, max_d=9, max_q=64)
    try:
        _refused(native, fresh.gp_loo)                                                        # never conditioned
    finally:
        fresh.close()


# ---- the optimiser classes: a call inside a run changes nothing -----------------------------------------------------------------
def _probing(base):
    class Probing(base):
        def optimize_acqf_and_get_observation(self):
            new = super().optimize_acqf_and_get_observation()
            self.seen.append((np.array(self.f_evals, dtype=np.float64), self.loo()))
            return new
    return Probing


@pytest.mark.parametrize("name", ["PCA_BO", "Vanilla_BO"])
def test_loo_inside_a_run(name):
    import Algorithms
    base = getattr(Algorithms, name)
    runs = []
    for cls in (base, _probing(base)):
        opt = cls(budget=12, n_DoE=8, random_seed=15051)
        opt.seen = []
        opt(problem=BBOBProblem(15, 0, 5), dim=5, bounds=np.array([-5.0, 5.0]))
        runs.append(opt)
    plain, probed = runs
    assert np.array(plain.x_evals).tobytes() == np.array(probed.x_evals).tobytes()
    assert np.array(plain.f_evals, dtype=np.float64).tobytes() == np.array(probed.f_evals, dtype=np.float64).tobytes()
    assert len(probed.seen) == 4
    for f, loo in probed.seen:
        assert all(loo[key].shape == f.shape for key in LR.KEYS)
        # entry i belongs to the i-th evaluated point: z_i is (f_i - mean_i) / sqrt(var_i)
        z = (f - loo["mean"]) / np.sqrt(loo["variance"])
        assert np.abs(z - loo["z"]).max() <= 1e-6 * max(1.0, np.abs(loo["z"]).max())
        assert np.isfinite(loo["lpd_sum"])
    with pytest.raises(RuntimeError):
        probed.loo()                                                                          # the run is over
