"""Appending points to the GPs of a lock-step batch on the MI355X and taking them back (pcabo_batch_gp_extend /
pcabo_batch_gp_truncate / pcabo_batch_gp_extended; Batch.gp_extend / gp_truncate / n_base): the B > 1 launches of k_ext_ks,
k_ext_append and k_ext_truncate (kernels_ext.hip) and the gated matrix-vector launches between them (launch_alpha_gated).

The yardstick is the single context: every run that takes part must end with the BYTES it has in a context of its own that was
conditioned (or fitted) on the same data and extended by pcabo_gp_extend with the same points - tests/test_gpu_extend.py judges that
arithmetic against the extended-precision reference, this file only compares bytes.  What a run that takes no part keeps, what a
failed pivot takes back and what the round trip promises are byte comparisons with the batch's own earlier answers.

A run that is set aside (its pivot failed, or it was parked during the extend) is refused by every model call; the reader
gp_state() of its member context, which launches nothing, still hands out its factors at the n it holds, so what the extend and the
truncate leave of it is read directly, before and after.

max_q: the issue sets 32 for the file.  The round-trip and optimiser tests use 128: with 32 the device-resident optimiser never
applies (its records lie behind 64 values of a run's value buffer) and pcabo_batch_device_acq_eval refuses; those tests assert that
the device path ran.

A run WITHOUT a GP beside extended ones (its batched conditioning failed), and an extend at a non-zero rung of the jitter ladder, are
in tests/test_gpu_batch_rare_paths.py (test_one_run_ends_without_a_gp, test_downstream_of_a_climbed_run).
"""
import copy

import numpy as np
import pytest

import extend_reference as ER
import gp_reference as G
import pcabo_oracle as O
from ard_reference import ard_state

pytestmark = pytest.mark.gpu

B, MAX_N, MAX_D, MAX_Q = 3, 140, 8, 32
MAX_Q_OPT = 128                                                    # the device-resident optimiser keeps its records behind 64 values
OK, ERR_ARG, NOT_PD = 0, -1, -2
SENTINEL = -777.25
STATE_KEYS = ("L", "R", "alpha", "norm_bounds")
POST_KEYS = ("mean", "variance", "covariance")
LOO_KEYS = ("mean", "variance", "z", "lpd")
SHAPES = [(17, 1), (63, 3), (64, 1), (127, 3)]


# ---- data ------------------------------------------------------------------------------------------------------------------------
def _cases(n, k, hyper="default"):
    """B cases of n points with different data per run: the thirds of gp_reference.make_case("lhs", B n, k, hyper)."""
    base = G.make_case("lhs", B * n, k, hyper)
    out = []
    for b in range(B):
        c = copy.copy(base)
        c.n, c.Z, c.y = n, np.ascontiguousarray(base.Z[b * n:(b + 1) * n]), np.ascontiguousarray(base.y[b * n:(b + 1) * n])
        out.append(c)
    return out


def _kinds(p):
    return tuple(("uniform", "copy0")[i % 2] for i in range(p))


def _new_points(cases, p):
    """Per run p new points and values (extend_reference.new_points with the kinds uniform / copy0, on the run's own data)."""
    pts = [ER.new_points(c, ER.held_of(c)[0], _kinds(p)) for c in cases]
    return [x for x, _ in pts], np.stack([y + 3.0 * b for b, (_, y) in enumerate(pts)])


def _probes(case, q, seed):
    lo, hi = case.Z.min(axis=0), case.Z.max(axis=0)
    return np.random.default_rng([seed, case.n, case.k]).uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), size=(q, case.k))


def _best(case):
    return float(np.float32(np.median(case.y)))


def _kernel(native, case):
    return native.KERNEL_RBF if case.kernel == "rbf" else native.KERNEL_MATERN52


# ---- the two sides ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def singles(native):
    cs = [native.Context(max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q) for _ in range(B)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture()
def bt(native):
    b = native.Batch(B, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q)
    yield b
    b.close()


@pytest.fixture()
def bt_opt(native):
    """A batch with room for the device-resident optimiser (its modes are switched per call)."""
    b = native.Batch(B, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q_OPT)
    yield b
    b.close()


def _condition_batch(native, bt, cases, wait=True):
    c0 = cases[0]
    bt.gp_condition_begin(np.stack([c.Z for c in cases]), np.stack([c.y for c in cases]), norm_bounds=c0.norm_bounds,
                          lengthscale=c0.lengthscale, gp_noise=c0.noise, kernel=_kernel(native, c0))
    if wait:
        _, status = bt.gp_wait_eval([_probes(c, 4, 7) for c in cases], [_best(c) for c in cases])
        assert (status == OK).all()


def _condition_single(native, c, case):
    c.gp_condition(case.y, Z=case.Z, norm_bounds=case.norm_bounds, lengthscale=case.lengthscale, noise=case.noise,
                   kernel=_kernel(native, case))


def _state_bytes(st):
    return [st[key].tobytes() for key in STATE_KEYS] + [np.float64(st["y_mean"]).tobytes(), np.float64(st["y_std"]).tobytes()]


def _model_bytes(c, case):
    """State, posterior with covariance at 17 probes and the leave-one-out vectors of a single context (or a member used as one)."""
    post, loo = c.gp_posterior(_probes(case, 17, 2), covariance=True), c.gp_loo()
    return (_state_bytes(c.gp_state()) + [post[key].tobytes() for key in POST_KEYS] +
            [np.asarray(loo[key]).tobytes() for key in LOO_KEYS] + [np.float64(loo["lpd_sum"]).tobytes()])


def _batch_model_bytes(bt, cases, runs=None):
    """The same through the batch's calls, per run: gp_state() of the member, Batch.gp_posterior, Batch.gp_loo."""
    post = bt.gp_posterior([_probes(c, 17, 2) for c in cases], covariance=True)
    loo = bt.gp_loo()
    out = {}
    for b in (range(bt.B) if runs is None else runs):
        assert post[b] is not None and loo[b] is not None, b
        assert loo[b]["mean"].shape == (bt.n,)
        out[b] = (_state_bytes(bt.ctx[b].gp_state()) + [post[b][key].tobytes() for key in POST_KEYS] +
                  [loo[b][key].tobytes() for key in LOO_KEYS] + [np.float64(loo[b]["lpd_sum"]).tobytes()])
    return out


def _alone(native, singles, cases, Xp, yp, runs=None):
    """Every run in a context of its own: conditioned on its data, extended with its points; the bytes of _model_bytes."""
    out = {}
    for b in (range(B) if runs is None else runs):
        _condition_single(native, singles[b], cases[b])
        singles[b].gp_extend(Xp[b], None if yp is None else yp[b])
        out[b] = _model_bytes(singles[b], cases[b])
    return out


def _options(native, bt, group=None, device=None):
    if group is not None:
        bt._chk(native.LIB.pcabo_batch_set_option(bt._h, native.OPT_GROUP_ACQ, int(group)))
    if device is not None:
        bt._chk(native.LIB.pcabo_batch_set_option(bt._h, native.OPT_DEVICE_LBFGSB, int(device)))
        bt.device_lbfgsb = int(device)


def _starts(cases, boxes):
    return [np.random.default_rng([3, c.n, c.k, b]).uniform(boxes[b][0], boxes[b][1], size=(6, c.k)) for b, c in enumerate(cases)]


def _optimised(native, bt, cases, group, device):
    """Batch.optimize_acqf in one of its modes (6 restarts, batch_limit 3, fixed seeded starts): bytes per run, the status."""
    _options(native, bt, group=group, device=device)
    boxes = bt.acq_bounds()
    outs, status = bt.optimize_acqf(_starts(cases, boxes), boxes, [_best(c) for c in cases], batch_limit=3)
    if device == 1:
        assert len(bt.device_group_out()[0]) == 2                   # the call did run inside the one launch (raises otherwise)
    if device == 2:
        assert len(bt.twin_branches()[0]) == 2                      # ... or through its host-stepped twin
    return [[np.ascontiguousarray(a).tobytes() for a in outs[b][:3]] for b in range(bt.B)], status


MODES = [(1, 0), (0, 0), (1, 1)]                                   # (PCABO_OPT_GROUP_ACQ, PCABO_OPT_DEVICE_LBFGSB)


def _snapshot(native, bt, cases):
    """Everything the round trip promises, of every run."""
    out = [_batch_model_bytes(bt, cases)]
    for group, device in MODES:
        res, status = _optimised(native, bt, cases, group, device)
        assert (status == OK).all()
        out.append(res)
    val, grad = bt.device_acq_eval([_probes(c, 3, 1) for c in cases], [_best(c) for c in cases])      # (device mode is on here)
    out.append([v.tobytes() for v in val] + [g.tobytes() for g in grad])
    _options(native, bt, group=1, device=0)
    return out


# ---- 1. bit-equal to alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyper", ["default", "rbf"])
@pytest.mark.parametrize("n,p", SHAPES, ids=lambda v: str(v))
def test_every_run_equals_its_own_context(native, bt, singles, n, p, hyper):
    cases = _cases(n, 5, hyper)
    _condition_batch(native, bt, cases)
    assert bt.n_base == n == bt.n
    Xp, yp = _new_points(cases, p)
    new_n, status = bt.gp_extend(Xp, yp)
    assert new_n == n + p == bt.n and bt.n_base == n and (status == OK).all()
    assert all(c.n == n + p and c.n_base == n for c in bt.ctx)     # pcabo_gp_extended on a member reads the batch's counts
    assert _batch_model_bytes(bt, cases) == _alone(native, singles, cases, Xp, yp)
    # believer mode from the same start
    assert bt.gp_truncate() == n
    new_n, status = bt.gp_extend(Xp)
    assert new_n == n + p and (status == OK).all()
    assert _batch_model_bytes(bt, cases) == _alone(native, singles, cases, Xp, None)


def test_the_padding_is_written_over_stale_data(native, bt, singles):
    """64 -> 65 with a throw-away 130-point conditioning in front: the capacity buffers hold stale rows where the new block goes."""
    _condition_batch(native, bt, _cases(130, 5))
    for b, c in enumerate(_cases(130, 5)):
        _condition_single(native, singles[b], c)
    cases = _cases(64, 5)
    _condition_batch(native, bt, cases)
    Xp, yp = _new_points(cases, 1)
    _, status = bt.gp_extend(Xp, yp)
    assert (status == OK).all()
    assert _batch_model_bytes(bt, cases) == _alone(native, singles, cases, Xp, yp)


def test_more_points_than_the_staging_holds_at_once(native, bt, singles):
    """17 -> 67 at k = 5: max_q * max_d + 8 = 264 doubles hold 44 rows with their values, so the points travel in two chunks."""
    n, p = 17, 50
    cases = _cases(n, 5)
    _condition_batch(native, bt, cases)
    pts = [ER.new_points(c, ER.held_of(c)[0], ("uniform",) * p) for c in cases]
    Xp, yp = [x for x, _ in pts], np.stack([y for _, y in pts])
    new_n, status = bt.gp_extend(Xp, yp)
    assert new_n == n + p and (status == OK).all()
    assert _batch_model_bytes(bt, cases) == _alone(native, singles, cases, Xp, yp)
    assert bt.gp_truncate() == n


# ---- 2. runs of different k --------------------------------------------------------------------------------------------------------
def _embedded(seed, n, k, d=MAX_D):
    Z, y = ard_state(seed, n, k)
    rng = np.random.default_rng(9000 + seed)
    X = 1e-4 * rng.uniform(-2.0, 2.0, size=(n, d))
    X[:, :k] = Z
    return X, y, rng.normal(0, 1e-8, X.shape), np.argsort(np.argsort(y)).astype(np.int64) + 1


def test_runs_of_different_k(native, bt, singles):
    n, want_k, vt = 40, (5, 3, 1), 0.999
    X, y, noise, ranks = (np.stack(a) for a in zip(*[_embedded(11 + b, n, k) for b, k in enumerate(want_k)]))
    ks = [O.weighted_pca(X[b], y[b], False, vt, 0, noise=noise[b], ranks=ranks[b]).k for b in range(B)]      # chosen on the CPU
    assert len(set(ks)) >= 2, ks
    bt.wpca_gp_condition_begin(X, ranks, noise, y, var_threshold=vt)
    assert [r["k"] for r in bt.wpca_results()] == ks
    boxes = bt.acq_bounds()
    probes = [np.random.default_rng(40 + b).uniform(boxes[b][0], boxes[b][1], size=(17, ks[b])) for b in range(B)]
    _, status = bt.gp_wait_eval(probes, y.min(axis=1))
    assert (status == OK).all()
    Xp = [np.random.default_rng(50 + b).uniform(boxes[b][0], boxes[b][1], size=(2, ks[b])) for b in range(B)]      # packed with stride k_b
    yp = np.stack([y[b, :2] + 0.25 for b in range(B)])
    new_n, status = bt.gp_extend(Xp, yp)
    assert new_n == n + 2 and (status == OK).all()
    post, loo = bt.gp_posterior(probes, covariance=True), bt.gp_loo()
    for b, c in enumerate(singles):
        assert c.wpca_gp_condition(X[b], y[b], ranks=ranks[b], noise=noise[b], var_threshold=vt)["k"] == ks[b]
        c.gp_wait()
        c.gp_extend(Xp[b], yp[b])
        assert _state_bytes(bt.ctx[b].gp_state()) == _state_bytes(c.gp_state()), b
        one = c.gp_posterior(probes[b], covariance=True)
        assert all(post[b][key].tobytes() == one[key].tobytes() for key in POST_KEYS), b
        one = c.gp_loo()
        assert all(loo[b][key].tobytes() == one[key].tobytes() for key in LOO_KEYS), b


# ---- 3. after a fit ------------------------------------------------------------------------------------------------------------------
def test_after_a_fit_every_run_reads_its_own_model(native, bt, singles):
    """n = 20, k = 3: gp_fit, then gp_fit_ard (which also starts over from n_base); value and believer mode behind each."""
    n, k = 20, 3
    Z, y = (np.stack(a) for a in zip(*[ard_state(21 + b, n, k) for b in range(B)]))
    cases = [G.make_case("lhs", n, k) for _ in range(B)]
    for b, c in enumerate(cases):
        c.Z, c.y = Z[b], y[b]
    Xp = [np.random.default_rng(60 + b).uniform(-2.0, 2.0, size=(2, k)) for b in range(B)]
    yp = np.stack([y[b, :2] + 0.5 for b in range(B)])
    bt.gp_condition_begin(Z, y)
    for ard in (False, True):
        fits = bt.gp_fit_ard() if ard else bt.gp_fit()
        assert bt.n == n == bt.n_base and all(f["status"] == OK for f in fits)
        assert len({f["noise"] for f in fits}) == B                 # the runs' models differ
        for values in (yp, None):
            new_n, status = bt.gp_extend(Xp, values)
            assert new_n == n + 2 and (status == OK).all()
            got = _batch_model_bytes(bt, cases)
            for b, c in enumerate(singles):
                one = c.gp_fit_ard(y[b], Z=Z[b]) if ard else c.gp_fit(y[b], Z=Z[b])
                assert one["theta"].tobytes() == fits[b]["theta"].tobytes()
                c.gp_extend(Xp[b], None if values is None else values[b])
                assert got[b] == _model_bytes(c, cases[b]), (ard, values is None, b)
            if values is not None:
                assert bt.gp_truncate() == n


# ---- 4. round trip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(63, 3), (64, 1)], ids=lambda v: str(v))
def test_round_trip(native, bt_opt, n, p):
    bt = bt_opt
    cases = _cases(n, 5)
    _condition_batch(native, bt, cases)
    before = _snapshot(native, bt, cases)
    Xp, yp = _new_points(cases, p)
    bt.gp_extend(Xp, yp)
    assert _snapshot(native, bt, cases) != before
    assert bt.gp_truncate() == n == bt.n == bt.n_base
    assert _snapshot(native, bt, cases) == before
    assert bt.gp_truncate(n) == n                                   # n0 == n: nothing to do


def test_extend_extend_truncate_to_the_first(native, bt):
    n = 63
    cases = _cases(n, 5)
    _condition_batch(native, bt, cases)
    Xp, yp = _new_points(cases, 3)
    bt.gp_extend([x[:1] for x in Xp], yp[:, :1])
    first = _batch_model_bytes(bt, cases)
    bt.gp_extend([x[1:] for x in Xp], yp[:, 1:])
    assert bt.n == n + 3 and bt.n_base == n
    assert bt.gp_truncate(n + 1) == n + 1
    assert _batch_model_bytes(bt, cases) == first
    bt.gp_extend([x[1:] for x in Xp], yp[:, 1:])                   # three points in two calls or in one: the same bytes
    two_calls = _batch_model_bytes(bt, cases)
    bt.gp_truncate()
    bt.gp_extend(Xp, yp)
    assert _batch_model_bytes(bt, cases) == two_calls
    _condition_batch(native, bt, cases)                             # a new conditioning starts over
    assert bt.n == n == bt.n_base


# ---- 5. the optimiser sees the extended model ------------------------------------------------------------------------------------
def test_the_optimiser_sees_the_extended_model(native, singles):
    cases = _cases(64, 5)
    Xp, yp = _new_points(cases, 1)
    bt = native.Batch(B, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q_OPT, device_lbfgsb=1)
    try:
        _condition_batch(native, bt, cases)                         # (the transposed root inverse of the 64 points is built here)
        bt.gp_extend(Xp, yp)
        device, status = _optimised(native, bt, cases, 1, 1)
        assert (status == OK).all()
        twin, status = _optimised(native, bt, cases, 1, 2)          # the host-driven twin, in the same batch
        assert (status == OK).all()
        assert device == twin
        for b, c in enumerate(singles):
            _condition_single(native, c, cases[b])
            c.gp_extend(Xp[b], yp[b])
        boxes = bt.acq_bounds()
        starts = _starts(cases, boxes)
        for group in (1, 0):
            got, status = _optimised(native, bt, cases, group, 0)
            assert (status == OK).all()
            for b, c in enumerate(singles):
                c.set_option(native.OPT_GROUP_ACQ, group)
                try:
                    cand, vals, _, _ = c.optimize_acqf(starts[b], boxes[b], _best(cases[b]), batch_limit=3)
                finally:
                    c.set_option(native.OPT_GROUP_ACQ, 0)
                assert got[b][0] == cand.tobytes() and got[b][1] == vals.tobytes(), (group, b)
    finally:
        bt.close()


# ---- 6. who takes part ---------------------------------------------------------------------------------------------------------------
def _refused(native, call, code=ERR_ARG):
    with pytest.raises(native.PcaboError) as e:
        call()
    assert e.value.code == code
    return str(e.value)


def test_a_parked_run_keeps_its_bytes(native, bt, singles):
    n, p = 63, 3
    cases = _cases(n, 5)
    _condition_batch(native, bt, cases)
    entry = _state_bytes(bt.ctx[1].gp_state())
    bt.set_active([1, 0, 1])
    Xp, yp = _new_points(cases, p)
    Xp[1] = None                                                    # its blocks are not read: no points, and a NaN among its values
    yp[1] = np.nan
    new_n, status = bt.gp_extend(Xp, yp)
    assert new_n == n + p and list(status) == [OK, ERR_ARG, OK]
    assert _batch_model_bytes(bt, cases, (0, 2)) == _alone(native, singles, cases, Xp, yp, (0, 2))
    assert bt.ctx[1].n == n and bt.ctx[0].n == n + p
    assert _state_bytes(bt.ctx[1].gp_state()) == entry              # read directly: the extend wrote none of its bytes
    _refused(native, lambda: bt.ctx[1].gp_loo())                    # out of step: at n_base while its batch is at n + p
    _refused(native, lambda: bt.set_active([1, 1, 1]))              # nobody changes sides while points are appended
    bt.set_active([1, 0, 1])                                        # (the same flags: nothing changes)
    assert bt.gp_truncate() == n
    assert _state_bytes(bt.ctx[1].gp_state()) == entry              # ... and neither did the truncate
    bt.set_active([1, 1, 1])
    assert bt.gp_posterior([_probes(c, 17, 2) for c in cases])[1] is not None


# ---- 7. a pivot that fails in one run only ---------------------------------------------------------------------------------------
def _raw_posterior(native, bt, cases, q=5):
    mean, var, status = np.full((B, q), SENTINEL), np.full((B, q), SENTINEL), np.full(B, 77, dtype=np.int32)
    buf = np.zeros((B, q * MAX_D))
    for b, c in enumerate(cases):
        buf[b, : q * c.k] = _probes(c, q, 2).ravel()
    bt._chk(native.LIB.pcabo_batch_gp_posterior(bt._h, native._ptr(buf), q, 0, native._ptr(mean), native._ptr(var), None,
                                                native._ptr(status)))
    return mean, var, status


def _raw_loo(native, bt):
    mean, total, status = np.full((B, bt.n), SENTINEL), np.full(B, SENTINEL), np.full(B, 77, dtype=np.int32)
    bt._chk(native.LIB.pcabo_batch_gp_loo(bt._h, native._ptr(mean), None, None, None, native._ptr(total), native._ptr(status)))
    return mean, total, status


@pytest.mark.parametrize("believer", [False, True], ids=["values-second-of-three", "believer-first-of-three"])
def test_a_pivot_that_fails_in_one_run_only(native, bt, singles, believer):
    """Nothing is provoked on the device: a finite point at 1e200 in every coordinate, whose normalised squared distance overflows,
    so ks and d2 are NaN (the input of test_gpu_extend.py's test_not_positive_definite_is_taken_back).  n = 63: NP grows."""
    n, p = 63, 3
    cases = _cases(n, 5)
    _condition_batch(native, bt, cases)
    before = _batch_model_bytes(bt, cases)
    Xp, yp = _new_points(cases, p)
    Xp[1] = Xp[1].copy()
    Xp[1][0 if believer else 1] = 1e200
    values = None if believer else yp
    new_n, status = bt.gp_extend(Xp, values)
    assert new_n == n + p and list(status) == [OK, NOT_PD, OK]
    assert "positive definite" in bt._err() and "run 1" in bt._err()
    assert _batch_model_bytes(bt, cases, (0, 2)) == _alone(native, singles, cases, Xp, values, (0, 2))
    # run 1 is set aside: its state bytes are those of entry (read directly), it is skipped by every call, its output blocks left alone
    assert bt.ctx[1].n == n and _state_bytes(bt.ctx[1].gp_state()) == before[1][:6]
    _refused(native, lambda: bt.ctx[1].gp_loo())
    _refused(native, lambda: bt.ctx[1].gp_posterior(_probes(cases[1], 3, 2)))
    mean, var, st = _raw_posterior(native, bt, cases)
    assert list(st) == [OK, ERR_ARG, OK] and (mean[1] == SENTINEL).all() and (var[1] == SENTINEL).all() and (mean[0] != SENTINEL).all()
    mean, total, st = _raw_loo(native, bt)
    assert list(st) == [OK, ERR_ARG, OK] and (mean[1] == SENTINEL).all() and total[1] == SENTINEL
    assert bt.gp_posterior([_probes(c, 17, 2) for c in cases])[1] is None and bt.gp_loo()[1] is None
    again, status = bt.gp_extend([x[:1] for x in _new_points(cases, 1)[0]], yp[:, :1])
    assert again == n + p + 1 and list(status) == [OK, ERR_ARG, OK]
    assert bt.gp_truncate(n + p) == n + p                           # not far enough back for run 1
    assert _state_bytes(bt.ctx[1].gp_state()) == before[1][:6]
    _refused(native, lambda: bt.ctx[1].gp_loo())
    assert _batch_model_bytes(bt, cases, (0, 2)) == _alone(native, singles, cases, Xp, values, (0, 2))
    # back to n_base: all three as before the extend, run 1 live again
    assert bt.gp_truncate() == n
    assert _batch_model_bytes(bt, cases) == before
    fine = _new_points(cases, p)[0]
    new_n, status = bt.gp_extend(fine, yp)                          # and the batch goes on, run 1 with it
    assert new_n == n + p and (status == OK).all()
    assert _batch_model_bytes(bt, cases) == _alone(native, singles, cases, fine, yp)


def test_a_failed_run_is_brought_back_below_the_n_it_holds(native, bt):
    """63 -> 64 for all, then three more of which run 1 fails the second: it is set aside at 64.  truncate(64) brings it back with
    nothing to take back; truncate(63) from the same state takes its one row back with the others' (k_ext_truncate for a run that
    holds fewer rows than its batch)."""
    n = 63
    cases = _cases(n, 5)
    _condition_batch(native, bt, cases)
    before = _batch_model_bytes(bt, cases)
    Xp, yp = _new_points(cases, 4)
    one = ([x[:1] for x in Xp], yp[:, :1])
    rest = [x[1:].copy() for x in Xp]
    rest[1][1] = 1e200
    bt.gp_extend(*one)
    first = _batch_model_bytes(bt, cases)
    for back_to, want in ((n + 1, first), (n, before)):
        _, status = bt.gp_extend(rest, yp[:, 1:])
        assert list(status) == [OK, NOT_PD, OK] and bt.n == n + 4
        assert bt.ctx[1].n == n + 1 and _state_bytes(bt.ctx[1].gp_state()) == first[1][:6]
        assert bt.gp_truncate(back_to) == back_to
        assert _batch_model_bytes(bt, cases) == want, back_to
    assert bt.n == n == bt.n_base


def test_a_scoring_of_the_extended_batch_leaves_a_run_aside(native, bt):
    """After a fit the batch can be scored (gp_wait_eval) while points are appended - the look-ahead score.  A run set aside is
    skipped by it, its block of values left alone, and stays aside for the calls that follow."""
    n, k, q = 20, 3, 4
    Z, y = (np.stack(a) for a in zip(*[ard_state(21 + b, n, k) for b in range(B)]))
    bt.gp_condition_begin(Z, y)
    assert all(f["status"] == OK for f in bt.gp_fit())
    Xp = [np.random.default_rng(60 + b).uniform(-2.0, 2.0, size=(2, k)) for b in range(B)]
    Xp[1][0] = 1e200
    _, status = bt.gp_extend(Xp, np.stack([y[b, :2] + 0.5 for b in range(B)]))
    assert list(status) == [OK, NOT_PD, OK]
    probes = [np.random.default_rng(70 + b).uniform(-2.0, 2.0, size=(q, k)) for b in range(B)]
    buf = np.zeros((B, q * MAX_D))
    for b in range(B):
        buf[b, : q * k] = probes[b].ravel()
    best, val, st = np.ascontiguousarray(y.min(axis=1)), np.full((B, q), SENTINEL), np.full(B, 77, dtype=np.int32)
    bt._chk(native.LIB.pcabo_batch_gp_condition_end_eval(bt._h, native._ptr(buf), q, native._ptr(best), 0, native.ACQ_LOG_EI,
                                                         native._ptr(val), native._ptr(st)))
    assert list(st) == [OK, ERR_ARG, OK] and (val[1] == SENTINEL).all() and (val[0] != SENTINEL).all() and (val[2] != SENTINEL).all()
    post = bt.gp_posterior(probes)
    assert post[1] is None and post[0] is not None and post[2] is not None
    assert bt.gp_loo()[1] is None
    _, status = bt.gp_extend([x[1:] for x in Xp], None)
    assert list(status) == [OK, ERR_ARG, OK]
    _refused(native, lambda: bt.ctx[1].gp_loo())
    assert bt.gp_truncate() == n
    assert all(p is not None for p in bt.gp_posterior(probes))


def test_a_batch_of_one_run(native, singles):
    """B = 1 is still a batch: its run keeps a header with the skip word, the gated matrix-vector launches and the strided copies.
    With the module's B = 3 nothing would notice a batch of one run taking the single context's branches.  n = 63, p = 2: the second
    point opens a new 64-block.  The failing input is the far-away finite point of test_a_pivot_that_fails_in_one_run_only."""
    n, p = 63, 2
    cases = _cases(n, 5)[:1]
    Xp, yp = _new_points(cases, p)
    bt = native.Batch(1, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q)
    try:
        _condition_batch(native, bt, cases)
        before = _batch_model_bytes(bt, cases)
        entry = _state_bytes(bt.ctx[0].gp_state())                 # L, R, alpha, the Normalize bounds, the Standardize statistics
        assert entry == before[0][:6]
        # (a) the run parked: it takes no part, the extend and the truncate write none of its bytes
        bt.set_active([0])
        new_n, status = bt.gp_extend(Xp, yp)
        assert new_n == n + p and list(status) == [ERR_ARG] and bt.ctx[0].n == n
        assert _state_bytes(bt.ctx[0].gp_state()) == entry
        assert bt.gp_truncate() == n
        assert _state_bytes(bt.ctx[0].gp_state()) == entry
        bt.set_active([1])
        assert _batch_model_bytes(bt, cases) == before
        # (b) the run active, values given; (c) believer mode: the bytes of a single context, and those of before once taken back
        for values in (yp, None):
            new_n, status = bt.gp_extend(Xp, values)
            assert new_n == n + p == bt.ctx[0].n and bt.n_base == n and list(status) == [OK]
            assert _batch_model_bytes(bt, cases) == _alone(native, singles, cases, Xp, values, (0,)), values is None
            assert bt.gp_truncate() == n
            assert _batch_model_bytes(bt, cases) == before, values is None
        # (d) a pivot that fails (the second point: ks and d2 are NaN): the run is taken back to the bytes of entry and set aside
        bad = [Xp[0].copy()]
        bad[0][1] = 1e200
        new_n, status = bt.gp_extend(bad, yp)
        assert new_n == n + p and list(status) == [NOT_PD] and bt.ctx[0].n == n
        assert "run 0" in bt._err() and "new point 1" in bt._err() and "positive definite" in bt._err()
        assert _state_bytes(bt.ctx[0].gp_state()) == entry
        _refused(native, lambda: bt.ctx[0].gp_loo())
        assert bt.gp_posterior([_probes(cases[0], 17, 2)])[0] is None
        assert bt.gp_truncate(n) == n                               # ... and live again
        assert _batch_model_bytes(bt, cases) == before
    finally:
        bt.close()


def test_a_refused_fit_leaves_the_extension_alone(native, bt):
    """pcabo_batch_gp_fit_ard with too small an ld_theta on an extended batch: refused, and n, n_base and every run's bytes stay."""
    n, k = 20, 3
    Z, y = (np.stack(a) for a in zip(*[ard_state(21 + b, n, k) for b in range(B)]))
    cases = [G.make_case("lhs", n, k) for _ in range(B)]
    for b, c in enumerate(cases):
        c.Z, c.y = Z[b], y[b]
    bt.gp_condition_begin(Z, y)
    bt.gp_fit()
    bt.gp_extend([np.random.default_rng(60 + b).uniform(-2.0, 2.0, size=(2, k)) for b in range(B)])
    state = _batch_model_bytes(bt, cases)
    th, out, info = np.zeros((B, 2 + k)), np.zeros(B), np.zeros((B, 4), dtype=np.int32)
    rc = native.LIB.pcabo_batch_gp_fit_ard(bt._h, native._ptr(th), 1 + k, native._ptr(out), native._ptr(info), None)
    assert rc == ERR_ARG and "ld_theta" in bt._err()
    assert bt._counts() == (n, n + 2) and all(c.n_base == n for c in bt.ctx)
    assert _batch_model_bytes(bt, cases) == state
    assert bt.gp_truncate() == n


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_run_alone(native, singles):
    n = 64
    cases = _cases(n, 3)
    bt = native.Batch(B, max_n=70, max_d=MAX_D, max_q=MAX_Q)
    L, ptr = native.LIB, native._ptr
    good, vals = np.zeros((B, 7 * MAX_D)), np.full((B, 7), 900.0)
    for b, c in enumerate(cases):
        good[b, : 7 * 3] = (c.Z[:7] + 0.01).ravel()
    try:
        _refused(native, lambda: bt._chk(L.pcabo_batch_gp_extend(bt._h, ptr(good), ptr(vals), 1, 0, None)))      # no conditioned batch
        _refused(native, lambda: bt._chk(L.pcabo_batch_gp_truncate(bt._h, 0, None)))
        _condition_batch(native, bt, cases)
        state = _batch_model_bytes(bt, cases)

        def unchanged():
            assert bt.n_base == n and bt._counts() == (n, n) and _batch_model_bytes(bt, cases) == state

        def raw(Z, y, p, flags):
            stride = np.zeros((B, max(p, 1) * MAX_D)) if Z is not None else None
            if Z is not None:
                for b in range(B):
                    stride[b, : max(p, 0) * 3] = Z[b, : max(p, 0) * 3]
            yy = None if y is None else np.ascontiguousarray(y[:, : max(p, 1)])
            bt._chk(L.pcabo_batch_gp_extend(bt._h, ptr(stride), ptr(yy), p, flags, None))

        _refused(native, lambda: raw(good, vals, 0, 0))                                       # p < 1
        _refused(native, lambda: raw(good, vals, -3, 0))
        _refused(native, lambda: raw(good, vals, 7, 0))                                       # n + p = max_n + 1
        _refused(native, lambda: raw(None, vals, 1, 0))                                       # Zp NULL
        _refused(native, lambda: raw(good, None, 1, 0))                                       # yp NULL without the believer flag
        _refused(native, lambda: raw(good, vals, 1, 2))                                       # unknown flag bits
        _refused(native, lambda: raw(good, vals, 1, 1 | 4))
        unchanged()
        for bad_value in (np.nan, np.inf):
            Zb, yb = good.copy(), vals.copy()
            Zb[2, 4] = bad_value
            _refused(native, lambda: raw(Zb, vals, 3, 0))                                     # a coordinate of a live run
            yb[1, 1] = bad_value
            _refused(native, lambda: raw(good, yb, 2, 0))                                     # a value of a live run
        unchanged()
        _refused(native, lambda: bt.gp_truncate(n - 1))                                       # n0 outside n_base .. n
        _refused(native, lambda: bt.gp_truncate(n + 1))
        msg = _refused(native, lambda: bt.ctx[0].gp_extend(cases[0].Z[:1] + 0.01, [900.0]))   # the single form on a member context
        assert "pcabo_gp_extend: the context belongs to a batch" in msg                      # (tests/test_gpu_call_order.py pins the text)
        msg = _refused(native, lambda: bt.ctx[0].gp_truncate(n))
        assert "pcabo_gp_truncate: the context belongs to a batch" in msg
        unchanged()
        _condition_batch(native, bt, cases, wait=False)
        _refused(native, lambda: raw(good, vals, 1, 0))                                       # between _begin and its end
        _refused(native, lambda: bt._chk(L.pcabo_batch_gp_truncate(bt._h, n, None)))
        _, status = bt.gp_wait_eval([_probes(c, 4, 7) for c in cases], [_best(c) for c in cases])
        assert (status == OK).all()
        unchanged()
        new_n, status = bt.gp_extend([c.Z[:6] + 0.01 for c in cases], vals[:, :6])            # n + p = max_n is accepted
        assert new_n == 70 and (status == OK).all()
        _refused(native, lambda: raw(good, vals, 1, 0))                                       # ... and nothing fits behind it
        _refused(native, lambda: bt.gp_truncate(71))
        assert bt.gp_truncate() == n
        unchanged()
    finally:
        bt.close()
