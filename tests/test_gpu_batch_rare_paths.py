"""The rare paths of a lock-step batch on the MI355X: ONE run of it leaves rung 0 of the jitter ladder, or ends without a GP, beside
runs that do neither.  This is host sequencing around kernels that other files judge - batch_score_collect's "redo it alone"
(factor_attempts on a member context, launch_factorisation with the member's own n, NP, k, noise and kernel, launch_rt_build in device
mode, pcabo_acq_eval on the member), its twin in batch_mll_round (mll_attempts), the rung a member keeps (RunOwn::rung) and what every
later batched call does with a run whose conditioning failed (RunOwn::have_gp == false) - so the yardsticks are the project's standing
ones: a run's bytes in a batch are its bytes in a context of its own, and the units of tests/gp_reference.py and
tests/extend_reference.py where a number is judged.

Inputs: tests/batch_rare_cases.py; tests/test_batch_rare_cases_cpu.py shows without a GPU that `retry`, `retry-tail` and the middle run
of the wPCA inputs fail rung 0 and factor at 1e-8 with a margin of 1e3, that the plain runs factor at rung 0 with that margin and that
`dead` has no rung at all.  Every test here still ASSERTS the rung (read off the run's own factor: the median of diag(L L^T) - diag(K)
within 1e-12 of a rung) or the status it is there for: a test that did not take the rare path fails.

Nothing is provoked on the device: a failed factorisation is an arithmetic outcome reported through an info word and a status, and all
inputs are finite and pass the host's argument checks.

A  test_one_run_climbs_the_ladder            Z given; B = 3 (plain, retry, plain), the same at capacity 321 with the 64 + 66-row tail
                                             (ld = 384 > NP = 192), and B = 86 (B nblk = 258 > 256: k_chol_lookn) with the rare run at
                                             7 and 85; host-paced, device and twin batches; log-EI and UCB at q = 70 and q = 16
B  test_the_fused_wpca_route_climbs          runs of k = 5, 3, 4, the middle one with duplicate rows
C  test_downstream_of_a_climbed_run          posterior, samples, LOO, acq_score, device_acq_eval, the optimiser in its three modes,
   test_downstream_on_the_fused_route        extend by 1 (values) and 3 (believer), truncate; inverse_map on route B
D  test_extend_at_a_rung_against_the_reference   a single context at rung 1e-8, rows n .. in extend_reference units with that rung
E  test_one_run_ends_without_a_gp            B = 3 (plain, dead, plain) through every call of C, gp_fit, and a clean conditioning after
   test_a_dead_run_in_the_oversubscribed_batch   B = 86, dead at 7: conditioning and scoring
F  test_the_lockstep_likelihood_redoes_a_run_alone   pcabo_batch_gp_mll's domain is s2 > 0, finite (mll_theta_ok, host_side.h): it admits
                                             1e-300, at which 1 + s2 == 1 and K is the K of noise 0, so the branch behind
                                             `if (c->hm->chol_info == 0) ... continue;` in batch_mll_round is reached without widening it
G  test_the_driver_parks_a_run_whose_conditioning_fails   pcabo/batchrun.py's "GP conditioning failed" line.  BatchedVanillaBO passes
                                             identity bounds (no range is taken from the data) and BatchedPCABO rotates the points first,
                                             so ONE constant coordinate fails neither; every stored coordinate of run 1 is overwritten
                                             instead - its centred data are then equal rows, the projected points have no range in any
                                             column, and the Normalize of BatchedPCABO (bounds from the data) divides 0 by 0

"Alone" for the device-resident optimiser and pcabo_batch_device_acq_eval, which a single context does not have, is a batch of B = 1
with the option set, conditioned on the run's data.
"""
import time
import warnings

import numpy as np
import pytest

import batch_rare_cases as BC
import extend_reference as ER
import gp_reference as G
from pcabo.bbob import BBOBProblem
from wpca_reference import EPS, f64, hp

pytestmark = pytest.mark.gpu

OK, ERR_ARG, NOT_PD = 0, -1, -2
LIMIT = 16.0
SENTINEL = -777.25
MAX_N, MAX_D, MAX_Q = 140, 8, 128                                  # room for 3 appended points; the device optimiser's records lie
BIG_N = 321                                                        # behind 64 values of a run's value buffer
BIG_B, BIG_RARE = 86, (7, 85)
ACQS = ("log_ei", "ucb")
QS = (70, 16)                                                      # the GEMM scoring (q >= 64) and the per-query kernels
STATE_KEYS = ("L", "R", "alpha", "norm_bounds")
POST_KEYS = ("mean", "variance", "covariance")
LOO_KEYS = ("mean", "variance", "z", "lpd")
SEEN = []                                                          # (what, run, rung or status): the summary the last test prints
_ALONE = {}


# ---- reading a model ---------------------------------------------------------------------------------------------------------------
def _raw_state(native, c):
    """pcabo_get_gp_state as it is: the whole n x n blocks of L and R, upper triangles included."""
    n, k = c.n, c.k
    L, R, alpha, ys, nb = np.empty((n, n)), np.empty((n, n)), np.empty(n), np.empty(2), np.empty((2, k))
    c._chk(native.LIB.pcabo_get_gp_state(c._h, *[native._ptr(a) for a in (L, R, alpha, ys, nb)]))
    return {"L": L, "R": R, "alpha": alpha, "y_mean": ys[0], "y_std": ys[1], "norm_bounds": nb}


def _state_bytes(st):
    return [st[key].tobytes() for key in STATE_KEYS] + [np.float64(st["y_mean"]).tobytes(), np.float64(st["y_std"]).tobytes()]


def _rung(st, K):
    """The rung a factor was accepted on, read off the factor itself."""
    seen = float(np.median((st["L"] * st["L"]).sum(axis=1) - np.diag(K)))
    rung = min(G.RUNGS, key=lambda r: abs(r - seen))
    assert abs(seen - rung) <= 1e-12, (seen, rung)
    return rung


def _scalar(native, case, acq):
    return (native.ACQ_LOG_EI, BC.best_of(case)) if acq == "log_ei" else (native.ACQ_UCB, 1.5)


def _options(native, bt, group=None, device=None):
    if group is not None:
        bt._chk(native.LIB.pcabo_batch_set_option(bt._h, native.OPT_GROUP_ACQ, int(group)))
    if device is not None:
        bt._chk(native.LIB.pcabo_batch_set_option(bt._h, native.OPT_DEVICE_LBFGSB, int(device)))
        bt.device_lbfgsb = int(device)


@pytest.fixture(scope="module")
def single(native):
    c = native.Context(max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q)
    t0 = time.time()
    yield c
    c.close()
    print("\ntest_gpu_batch_rare_paths: %.1f s between the shared context's creation and close" % (time.time() - t0))


def _alone(native, c, case, acq, q):
    """A run in a context of its own: conditioned on its data with the scoring enqueued behind it (gp_wait_eval).  Computed once per
    (case, acquisition, q) and never modified: the values' bytes, the state, the rung."""
    key = (case.id, acq, q)
    if key not in _ALONE:
        code, scalar = _scalar(native, case, acq)
        c.gp_condition(case.y, Z=case.Z, noise=case.noise, wait=False)
        val = c.gp_wait_eval(BC.probes(case, q), scalar, acq=code)
        st = _raw_state(native, c)
        model = _ALONE.setdefault(case.id, {"bytes": _state_bytes(st), "rung": _rung(st, c.gram())})
        assert model["bytes"] == _state_bytes(st)                   # (the model does not depend on what is scored behind it)
        _ALONE[key] = {"val": val.tobytes(), **model}
    return _ALONE[key]


def _condition_and_score(native, bt, cases, acq, q):
    """gp_condition_begin -> gp_wait_eval of a batch on the runs' own data; (values, status)."""
    codes = [_scalar(native, c, acq) for c in cases]
    bt.gp_condition_begin(np.stack([c.Z for c in cases]), np.stack([c.y for c in cases]), gp_noise=0.0)
    return bt.gp_wait_eval([BC.probes(c, q) for c in cases], [s for _, s in codes], acq=codes[0][0])


# ---- A. one run climbs the ladder; Z is given ----------------------------------------------------------------------------------------
def _shape(name):
    """(cases, the rare runs, the batch's capacity)."""
    if name == "B3":
        return [BC.plain(0), BC.retry(), BC.plain(2)], (1,), MAX_N
    if name == "B3-tail-ld384":
        return [BC.plain(0), BC.retry_tail(), BC.plain(2)], (1,), BIG_N
    cases = [BC.plain(s) for s in range(BIG_B)]
    for b in BIG_RARE:
        cases[b] = BC.retry()
    return cases, BIG_RARE, BC.N


@pytest.mark.parametrize("device", [0, 1, 2], ids=["host-paced", "device", "twin"])
@pytest.mark.parametrize("shape", ["B3", "B3-tail-ld384", "B86"])
def test_one_run_climbs_the_ladder(native, single, shape, device, capsys):
    """What each shape is there for:

    - B3: the redo of a member between two runs that stay at rung 0 - launch_factorisation on the member's own record and stream, the
      separate root-inverse launches, launch_rt_build where the batch is in device or twin mode, pcabo_acq_eval on the member;
    - B3-tail-ld384: the same at capacity 321, ld = 384 > NP = 192, the singular part in the first tile alone - a redo that took NP or
      n for the leading dimension, or the batch's stride for the member's, rebuilds another K;
    - B86: B nblk = 258 > 256 work-groups, the k_chol_lookn form with its own info-word writes; the rare run at 7 and at 85 (the last
      block of the strided copies), two members redone in one collect.

    Per run: status 0; the whole n x n blocks of L and R, alpha, the Normalize bounds and the y statistics and the returned values are
    the bytes of a context of its own; the rare runs' rung is > 0 and the one their own context ended on, every other run is at rung 0.
    The rare run's factor is judged once per shape by gp_reference.judge_ladder at its rung (16 units)."""
    cases, rare, cap = _shape(shape)
    B = len(cases)
    bt = native.Batch(B, max_n=cap, max_d=MAX_D, max_q=MAX_Q, device_lbfgsb=device)
    t0, lines = time.time(), []
    try:
        for acq in ACQS:
            for q in QS:
                val, status = _condition_and_score(native, bt, cases, acq, q)
                assert (status == OK).all(), (acq, q, status)
                for b, case in enumerate(cases):
                    one = _alone(native, single, case, acq, q)
                    st = _raw_state(native, bt.ctx[b])
                    assert _state_bytes(st) == one["bytes"], (shape, acq, q, b)
                    assert val[b].tobytes() == one["val"], (shape, acq, q, b)
                    rung = _rung(st, bt.ctx[b].gram())
                    assert rung == one["rung"], (shape, acq, q, b, rung, one["rung"])
                    assert (rung > 0.0) == (b in rare), (shape, acq, q, b, rung)
        for b in rare[:1]:                                          # (the bytes are the single context's: judged once)
            st, K = _raw_state(native, bt.ctx[b]), bt.ctx[b].gram()
            j = G.judge_ladder(cases[b], K, st["L"], st["R"], st["alpha"], st["y_mean"], st["y_std"])
            assert j.finite and j.flags_ok and j.rung > 0.0
            assert all(v <= LIMIT for v in j.ratios.values()), (shape, j.rung, j.ratios)
            lines.append("  %s %s run %d: rung %g (seen %.3e)  %s" % (shape, ("host-paced", "device", "twin")[device], b, j.rung, j.seen,
                                                                     "  ".join("%s %.3g" % kv for kv in j.ratios.items())))
            SEEN.append(("A %s/%d climbs" % (shape, device), b, j.rung))
    finally:
        bt.close()
    with capsys.disabled():
        print("\n" + "\n".join(lines) + "\n  %.1f s" % (time.time() - t0))


# ---- B. the same through the fused wPCA route ------------------------------------------------------------------------------------------
WPCA_KEYS = ("data_mean", "pca_mean", "components", "evr")


def _wpca_batch(native, device=0):
    X, y, ranks, noise = BC.wpca_inputs()
    bt = native.Batch(3, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q, device_lbfgsb=device)
    bt.wpca_gp_condition_begin(X, ranks, noise, y, var_threshold=BC.VAR_THRESHOLD, gp_noise=0.0)
    return bt, (X, y, ranks, noise)


def _wpca_single(c, data, b):
    X, y, ranks, noise = data
    return c.wpca_gp_condition(X[b], y[b], ranks=ranks[b], noise=noise[b], var_threshold=BC.VAR_THRESHOLD, gp_noise=0.0)


def _box_probes(boxes, q, seed):
    return [np.random.default_rng([seed, q, b]).uniform(bx[0], bx[1], size=(q, bx.shape[1])) for b, bx in enumerate(boxes)]


@pytest.mark.parametrize("device", [0, 1], ids=["host-paced", "device"])
def test_the_fused_wpca_route_climbs(native, device, capsys):
    """pcabo_batch_wpca_gp_condition_begin: k lives on the device while the conditioning is enqueued and the runs differ in it (5, 3,
    4).  The middle run's redo takes k and KP from the member's record: a record that still held the batch's largest k, or last
    call's, would rebuild a different K and nobody would notice.  Every run - wPCA results, state, values - is the bytes of a context
    of its own driven through pcabo_wpca_gp_condition_begin; the middle run's rung is > 0 and its own context's, the others' 0."""
    bt, data = _wpca_batch(native, device)
    singles = [native.Context(max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q) for _ in range(3)]
    try:
        res = bt.wpca_results()
        assert [r["k"] for r in res] == list(BC.WPCA_K)
        for acq in ACQS:
            for q in QS:
                if (acq, q) != (ACQS[0], QS[0]):
                    bt.wpca_gp_condition_begin(data[0], data[2], data[3], data[1], var_threshold=BC.VAR_THRESHOLD, gp_noise=0.0)
                    res = bt.wpca_results()
                probes = _box_probes(bt.acq_bounds(), q, 3)
                code = native.ACQ_LOG_EI if acq == "log_ei" else native.ACQ_UCB
                scalars = [float(np.float32(np.median(data[1][b]))) if acq == "log_ei" else 1.5 for b in range(3)]
                val, status = bt.gp_wait_eval(probes, scalars, acq=code)
                assert (status == OK).all(), (acq, q, status)
                for b, c in enumerate(singles):
                    one = _wpca_single(c, data, b)
                    assert one["k"] == res[b]["k"]
                    assert all(one[key].tobytes() == res[b][key].tobytes() for key in WPCA_KEYS), (acq, q, b)
                    alone = c.gp_wait_eval(probes[b], scalars[b], acq=code)
                    assert val[b].tobytes() == alone.tobytes(), (acq, q, b)
                    st, own = _raw_state(native, bt.ctx[b]), _raw_state(native, c)
                    assert _state_bytes(st) == _state_bytes(own), (acq, q, b)
                    rung = _rung(st, bt.ctx[b].gram())
                    assert rung == _rung(own, c.gram()) and (rung > 0.0) == (b == 1), (acq, q, b, rung)
        SEEN.append(("B wPCA/%d climbs" % device, 1, _rung(_raw_state(native, bt.ctx[1]), bt.ctx[1].gram())))
    finally:
        bt.close()
        for c in singles:
            c.close()


# ---- C. everything downstream of a batch that holds a climbed run ------------------------------------------------------------------
def _starts(boxes, nr=5):
    return [np.random.default_rng([3, b, bx.shape[1]]).uniform(bx[0], bx[1], size=(nr, bx.shape[1])) for b, bx in enumerate(boxes)]


def _model_bytes_single(c, probes):
    post, loo = c.gp_posterior(probes, covariance=True), c.gp_loo()
    smp = c.gp_posterior_samples(probes, n_samples=3, seed=5)
    return ([post[key].tobytes() for key in POST_KEYS] + [np.asarray(loo[key]).tobytes() for key in LOO_KEYS] +
            [np.float64(loo["lpd_sum"]).tobytes(), smp["samples"].tobytes(), smp["mean"].tobytes(), np.float64(smp["jitter"]).tobytes()])


def _model_bytes_batch(native, bt, probes):
    post, loo = bt.gp_posterior(probes, covariance=True), bt.gp_loo()
    smp = bt.gp_posterior_samples(probes, n_samples=3, seed=5)
    assert all(r is not None for r in post + loo + smp)
    return [_state_bytes(_raw_state(native, bt.ctx[b])) + [post[b][key].tobytes() for key in POST_KEYS] +
            [loo[b][key].tobytes() for key in LOO_KEYS] +
            [np.float64(loo[b]["lpd_sum"]).tobytes(), smp[b]["samples"].tobytes(), smp[b]["mean"].tobytes(),
             np.float64(smp[b]["jitter"]).tobytes()] for b in range(bt.B)]


def _downstream(native, bt, singles, condition_single, probes17, probes70, probes32, boxes, scalars):
    """Every call of the list on a conditioned batch against contexts of their own (condition_single(b) conditions singles[b] on run
    b's data and waits); device mode against batches of one run (alone1[b])."""
    B = bt.B
    for b in range(B):
        condition_single(singles[b], b)
    # the model as conditioned
    before = _model_bytes_batch(native, bt, probes17)
    for b, c in enumerate(singles):
        assert before[b] == _state_bytes(_raw_state(native, c)) + _model_bytes_single(c, probes17[b]), b
    val, status = bt.acq_score(probes70, scalars)
    assert (status == OK).all()
    for b, c in enumerate(singles):
        assert val[b].tobytes() == c.acq_eval(probes70[b], scalars[b], grad=False).tobytes(), b
    # the optimiser, host-paced through both kernels
    starts = _starts(boxes)
    for group in (1, 0):
        _options(native, bt, group=group, device=0)
        outs, status = bt.optimize_acqf(starts, boxes, scalars, batch_limit=3)
        assert (status == OK).all(), (group, status)
        for b, c in enumerate(singles):
            c.set_option(native.OPT_GROUP_ACQ, group)
            try:
                cand, vals, info, _ = c.optimize_acqf(starts[b], boxes[b], scalars[b], batch_limit=3)
            finally:
                c.set_option(native.OPT_GROUP_ACQ, 0)
            assert outs[b][0].tobytes() == cand.tobytes() and outs[b][1].tobytes() == vals.tobytes() and \
                outs[b][2].tobytes() == info.tobytes(), (group, b)
    _options(native, bt, group=1)
    # the device-resident optimiser, its twin and the device's evaluation: each run against a batch of that run alone
    got = {}
    for mode in (1, 2):
        _options(native, bt, device=mode)
        outs, status = bt.optimize_acqf(starts, boxes, scalars, batch_limit=3)
        assert (status == OK).all(), (mode, status)
        assert len(bt.device_group_out()[0] if mode == 1 else bt.twin_branches()[0]) == 2      # the call did take that path
        got[mode] = [[np.ascontiguousarray(a).tobytes() for a in outs[b][:3]] for b in range(B)]
    assert got[1] == got[2]
    _options(native, bt, device=1)
    return before, got[1], _device_eval_bytes(bt, probes32, scalars), starts


def _device_eval_bytes(bt, probes32, scalars):
    dval, dgrad = bt.device_acq_eval(probes32, scalars)
    return [v.tobytes() for v in dval] + [g.tobytes() for g in dgrad]


def _extend_and_back(native, bt, singles, probes17, Xp, yp, n, before):
    """gp_extend by 1 point (values) and by 3 (believer) with gp_truncate behind each: the extended bytes are the single contexts',
    the bytes after the truncate those from before the extend."""
    for p, values in ((1, True), (3, False)):
        new_n, status = bt.gp_extend([x[:p] for x in Xp], yp[:, :p] if values else None)
        assert new_n == n + p and (status == OK).all(), (p, status)
        got = _model_bytes_batch(native, bt, probes17)
        for b, c in enumerate(singles):
            assert c.gp_extend(Xp[b][:p], yp[b, :p] if values else None) == n + p
            assert got[b] == _state_bytes(_raw_state(native, c)) + _model_bytes_single(c, probes17[b]), (p, b)
            assert c.gp_truncate() == n
        assert got != before
        assert bt.gp_truncate() == n == bt.n
        assert _model_bytes_batch(native, bt, probes17) == before, p


def _alone_in_device_mode(native, condition_batch1, b, probes32, boxes, scalars, starts):
    """Run b in a batch of its own with the device-resident optimiser: the optimiser's and the device evaluation's bytes."""
    one = native.Batch(1, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q, device_lbfgsb=1)
    try:
        condition_batch1(one, b)
        outs, status = one.optimize_acqf([starts[b]], [boxes[b]], [scalars[b]], batch_limit=3)
        assert (status == OK).all() and len(one.device_group_out()[0]) == 2
        dval, dgrad = one.device_acq_eval([probes32[b]], [scalars[b]])
        return [np.ascontiguousarray(a).tobytes() for a in outs[0][:3]], dval[0].tobytes(), dgrad[0].tobytes()
    finally:
        one.close()


def test_downstream_of_a_climbed_run(native):
    """B3 with the batch created in device mode (the redo rebuilds the member's transposed root inverse on the member's stream, and
    the reads of K for the rungs outdate it again - rt_stale): every later call on the batch that holds the climbed run gives every
    run the bytes it has alone, the climbed run at ITS rung (d2 = 1 + s2 + rung - |v|^2 in the extend: the header the host writes)."""
    cases, rare, cap = _shape("B3")
    n = BC.N
    bt = native.Batch(3, max_n=cap, max_d=MAX_D, max_q=MAX_Q, device_lbfgsb=1)
    singles = [native.Context(max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q) for _ in range(3)]
    try:
        _, status = _condition_and_score(native, bt, cases, "log_ei", 70)
        assert (status == OK).all()
        boxes, scalars = bt.acq_bounds(), [BC.best_of(c) for c in cases]
        probes17, probes70, probes32 = ([BC.probes(c, q, 2) for c in cases] for q in (17, 70, 32))
        first = _device_eval_bytes(bt, probes32, scalars)           # on the transposed root inverse the redo itself built
        rungs = [_rung(_raw_state(native, c), c.gram()) for c in bt.ctx]      # (reading K outdates it: the next launch rebuilds it)
        assert rungs[1] > 0.0 and rungs[0] == rungs[2] == 0.0, rungs
        pts = [BC.new_points(c, 3, b) for b, c in enumerate(cases)]
        Xp, yp = [x for x, _ in pts], np.stack([y for _, y in pts])

        def condition_single(c, b):
            c.gp_condition(cases[b].y, Z=cases[b].Z, noise=0.0)

        def condition_batch1(one, b):
            _, st = _condition_and_score(native, one, [cases[b]], "log_ei", 70)
            assert (st == OK).all()

        before, opt, dev, starts = _downstream(native, bt, singles, condition_single, probes17, probes70, probes32, boxes, scalars)
        assert dev == first                                         # the redo's own build and the batch's rebuild: the same bytes
        for b in range(3):
            o, dv, dg = _alone_in_device_mode(native, condition_batch1, b, probes32, boxes, scalars, starts)
            assert opt[b] == o and dev[b] == dv and dev[3 + b] == dg, b
        _extend_and_back(native, bt, singles, probes17, Xp, yp, n, before)
        assert [_rung(_raw_state(native, c), c.gram()) for c in bt.ctx] == rungs
        SEEN.append(("C downstream, climbs", 1, rungs[1]))
    finally:
        bt.close()
        for c in singles:
            c.close()


def test_downstream_on_the_fused_route(native):
    """The same behind pcabo_batch_wpca_gp_condition_begin (k = 5, 3, 4, the climbed run in the middle), with pcabo_batch_inverse_map."""
    bt, data = _wpca_batch(native, 1)
    singles = [native.Context(max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q) for _ in range(3)]
    n = BC.N
    try:
        assert [r["k"] for r in bt.wpca_results()] == list(BC.WPCA_K)
        boxes = bt.acq_bounds()
        scalars = [float(np.float32(np.median(data[1][b]))) for b in range(3)]
        probes17, probes70, probes32 = (_box_probes(boxes, q, 2) for q in (17, 70, 32))
        _, status = bt.gp_wait_eval(probes70, scalars)
        assert (status == OK).all()
        first = _device_eval_bytes(bt, probes32, scalars)
        rungs = [_rung(_raw_state(native, c), c.gram()) for c in bt.ctx]
        assert rungs[1] > 0.0 and rungs[0] == rungs[2] == 0.0, rungs
        Xp = [np.random.default_rng([50, b]).uniform(bx[0], bx[1], size=(3, bx.shape[1])) for b, bx in enumerate(boxes)]
        yp = np.stack([data[1][b, :3] + 0.25 for b in range(3)])

        def condition_single(c, b):
            assert _wpca_single(c, data, b)["k"] == BC.WPCA_K[b]
            c.gp_wait()

        def condition_batch1(one, b):
            one.wpca_gp_condition_begin(data[0][b:b + 1], data[2][b:b + 1], data[3][b:b + 1], data[1][b:b + 1],
                                        var_threshold=BC.VAR_THRESHOLD, gp_noise=0.0)
            assert one.wpca_results()[0]["k"] == BC.WPCA_K[b]
            _, st = one.gp_wait_eval([probes70[b]], [scalars[b]])
            assert (st == OK).all()

        before, opt, dev, starts = _downstream(native, bt, singles, condition_single, probes17, probes70, probes32, boxes, scalars)
        assert dev == first                                         # the redo's own build and the batch's rebuild: the same bytes
        for b in range(3):
            o, dv, dg = _alone_in_device_mode(native, condition_batch1, b, probes32, boxes, scalars, starts)
            assert opt[b] == o and dev[b] == dv and dev[3 + b] == dg, b
        z = [np.random.default_rng([60, b]).uniform(bx[0], bx[1]) for b, bx in enumerate(boxes)]
        x = bt.inverse_map(z)
        for b, c in enumerate(singles):
            assert x[b].tobytes() == c.inverse_map(z[b]).tobytes(), b
        _extend_and_back(native, bt, singles, probes17, Xp, yp, n, before)
        SEEN.append(("C downstream on the fused route, climbs", 1, rungs[1]))
    finally:
        bt.close()
        for c in singles:
            c.close()


# ---- D. extend at a non-zero rung in a single context, against the reference --------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3])
def test_extend_at_a_rung_against_the_reference(native, single, p, capsys):
    """`retry` conditioned in a context of its own (rung 1e-8, asserted), extended by uniform points with values: rows n .. of L and
    R against extend_reference.step on the DEVICE's own R, bounds and statistics with rung = the device's rung, alpha against the
    long-double R^T (R y_s), 16 units - the units and limit of test_gpu_extend.py, which never leaves rung 0.
    test_batch_rare_cases_cpu.py shows that a pivot formed without the rung is ~1500 units off on this input, so this test tells the
    two apart.  (Believer mode forms the same rows; its bytes at a rung are compared in test_downstream_of_a_climbed_run.)"""
    case = BC.retry()
    n = case.n
    single.gp_condition(case.y, Z=case.Z, noise=0.0)
    st0 = _raw_state(native, single)
    rung = _rung(st0, single.gram())
    assert rung > 0.0
    Xp, yp = BC.new_points(case, p)
    assert single.gp_extend(Xp, yp) == n + p
    st1 = _raw_state(native, single)
    single.gp_truncate()
    assert st1["L"][:n, :n].tobytes() == st0["L"].tobytes() and st1["R"][:n, :n].tobytes() == st0["R"].tobytes()
    assert np.all(np.triu(st1["L"], 1) == 0.0) and np.all(np.triu(st1["R"], 1) == 0.0)
    Z, worst = case.Z, {"L": 0.0, "R": 0.0}
    for i in range(p):
        m = n + i
        b = ER.step(st1["R"][:m, :m], Xp[i], Z, st0["norm_bounds"], case.lengthscale, case.noise, case.kernel, rung=rung)
        worst["L"] = max(worst["L"], ER.ratio(hp(st1["L"][m, :m + 1]) - b.L_row, b.units.L_row))
        worst["R"] = max(worst["R"], ER.ratio(hp(st1["R"][m, :m + 1]) - b.R_row, b.units.R_row))
        Z = np.vstack([Z, Xp[i:i + 1]])
    ys = (hp(np.concatenate([case.y, yp])) - hp(st0["y_mean"])) / hp(st0["y_std"])
    alpha_ref, unit = ER.alpha_units(st1["R"], ys, 2.0 * EPS * np.abs(f64(ys[n:])))
    worst["alpha"] = ER.ratio(hp(st1["alpha"]) - alpha_ref, unit)
    with capsys.disabled():
        print("\n  extend %d -> %d at rung %g: units %s" % (n, n + p, rung, " ".join("%s %.3f" % kv for kv in worst.items())))
    SEEN.append(("D extend +%d at a rung" % p, 0, rung))
    assert max(worst.values()) <= ER.LIMIT, worst


# ---- E. one run ends without a GP -----------------------------------------------------------------------------------------------------
def _filled(shape, dtype=np.float64):
    return np.full(shape, SENTINEL if dtype == np.float64 else 77, dtype=dtype)


def _packed(bt, rows):
    """rows[b]: q x k_b -> the (B, q * max_d) block array the library reads."""
    q = rows[0].shape[0]
    buf = np.zeros((bt.B, q * bt.max_d))
    for b, r in enumerate(rows):
        buf[b, : r.size] = np.ascontiguousarray(r, dtype=np.float64).ravel()
    return buf, q


def _raw_calls(native, bt, probes17, probes70, probes32, starts, boxes, scalars):
    """Every query of the list through the C entry points with the outputs filled with a sentinel first: {call: (arrays, status)}."""
    L, ptr, B = native.LIB, native._ptr, bt.B
    bf = np.ascontiguousarray(scalars, dtype=np.float64)
    out = {}
    buf, q = _packed(bt, probes17)
    mean, var, cov, st = _filled((B, q)), _filled((B, q)), _filled((B, q, q)), _filled(B, np.int32)
    bt._chk(L.pcabo_batch_gp_posterior(bt._h, ptr(buf), q, 0, ptr(mean), ptr(var), ptr(cov), ptr(st)))
    out["posterior"] = ([mean, var, cov], st)
    base = np.ascontiguousarray(np.broadcast_to(native.sample_base(q, 3, None, 5), (B, 3, q)))
    smp, mean, jit, st = _filled((B, 3, q)), _filled((B, q)), _filled(B), _filled(B, np.int32)
    bt._chk(L.pcabo_batch_gp_posterior_sample(bt._h, ptr(buf), q, 0, ptr(base), 3, ptr(smp), ptr(mean), ptr(jit), ptr(st)))
    out["samples"] = ([smp, mean, jit], st)
    n = bt.n
    arrs, total, st = [_filled((B, n)) for _ in range(4)], _filled(B), _filled(B, np.int32)
    bt._chk(L.pcabo_batch_gp_loo(bt._h, *[ptr(a) for a in arrs], ptr(total), ptr(st)))
    out["loo"] = (arrs + [total], st)
    bt.acq_score_begin(probes70, scalars)
    val, st = _filled((B, 70)), _filled(B, np.int32)
    bt._chk(L.pcabo_batch_acq_score_end(bt._h, 70, ptr(val), ptr(st)))
    out["acq_score"] = ([val], st)
    nr, ics, bnd = bt._pack_ics(starts, boxes)
    for name, group, device in (("optimise host-paced", 1, 0), ("optimise per-query", 0, 0), ("optimise device", 1, 1), ("optimise twin", 1, 2)):
        _options(native, bt, group=group, device=device)
        cand, vals = _filled((B, nr * bt.max_d)), _filled((B, nr))
        info, failed, st = _filled((B, 2, 4), np.int32), _filled(B, np.int32), _filled(B, np.int32)
        bt._chk(L.pcabo_batch_optimize_acqf(bt._h, ptr(ics), nr, 3, ptr(bnd), 200, ptr(bf), 0, native.ACQ_LOG_EI, ptr(cand), ptr(vals),
                                            ptr(info), ptr(failed), ptr(st)))
        if device == 1:
            assert len(bt.device_group_out()[0]) == 2
        if device == 2:
            assert len(bt.twin_branches()[0]) == 2
        out[name] = ([cand, vals, info], st)
    _options(native, bt, group=1, device=1)
    buf, q = _packed(bt, probes32)
    val, grad = _filled((B, q)), _filled((B, q * bt.max_d))
    bt._chk(L.pcabo_batch_device_acq_eval(bt._h, ptr(buf), q, ptr(bf), 0, native.ACQ_LOG_EI, ptr(val), ptr(grad)))
    out["device_acq_eval"] = ([val, grad], None)
    return out


def _untouched(a):
    return bool(np.all(a == (SENTINEL if a.dtype == np.float64 else 77)))


def _refused(native, call, code=ERR_ARG):
    with pytest.raises(native.PcaboError) as e:
        call()
    assert e.value.code == code, e.value


def test_one_run_ends_without_a_gp(native, single, capsys):
    """B = 3 in device mode, `dead` in the middle.  The yardstick first: a context of its own ends on PCABO_ERR_NOT_PD (-2) for it.
    In the batch pcabo_batch_gp_condition_end_eval gives [0, -2, 0] and leaves the dead run's values alone; from then on it is a run
    WITHOUT A GP: computed with the others by every batched call, reported with PCABO_ERR_ARG (the optimiser: PCABO_ERR_NOT_PD, as
    include/pcabo.h states for it), its output blocks left as they are - sentinels intact; the runs beside it get, byte for byte, what
    the same calls give a batch of those two alone.  A lock-step fit reports the dead run's failure and fits the others to their own
    fits' bytes; a conditioning of all three on plain data afterwards equals a fresh batch's: the failure left nothing behind."""
    cases = [BC.plain(0), BC.dead(1), BC.plain(2)]
    n, live = BC.N, (0, 2)
    with pytest.raises(native.PcaboError) as err:
        single.gp_condition(cases[1].y, Z=cases[1].Z, noise=0.0)
    assert err.value.code == NOT_PD
    bt = native.Batch(3, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q, device_lbfgsb=1)
    two = native.Batch(2, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q, device_lbfgsb=1)
    try:
        for acq in ACQS:
            for q in QS:
                codes = [_scalar(native, c, acq) for c in cases]
                bt.gp_condition_begin(np.stack([c.Z for c in cases]), np.stack([c.y for c in cases]), gp_noise=0.0)
                buf, _ = _packed(bt, [BC.probes(c, q) for c in cases])
                val, status, bf = _filled((3, q)), _filled(3, np.int32), np.array([s for _, s in codes], dtype=np.float64)
                bt._chk(native.LIB.pcabo_batch_gp_condition_end_eval(bt._h, native._ptr(buf), q, native._ptr(bf), 0, codes[0][0],
                                                                     native._ptr(val), native._ptr(status)))
                assert list(status) == [OK, NOT_PD, OK], (acq, q, status)
                assert _untouched(val[1]), (acq, q)
                for b in live:
                    one = _alone(native, single, cases[b], acq, q)
                    assert _state_bytes(_raw_state(native, bt.ctx[b])) == one["bytes"] and val[b].tobytes() == one["val"], (acq, q, b)
                _refused(native, lambda: bt.ctx[1].gp_state())      # the call-order error: the member holds no model
        SEEN.append(("E B3 dead", 1, int(status[1])))
        _, status = _condition_and_score(native, two, [cases[b] for b in live], "ucb", QS[-1])
        assert (status == OK).all()
        # every query of the list: the dead run reported and left alone, the others as in the batch of two
        boxes3, scalars = bt.acq_bounds(), [BC.best_of(c) for c in cases]
        boxes3[1] = np.vstack([np.zeros(BC.K), np.ones(BC.K)])      # (the dead run's own box is NaN; its block is not read)
        probes17, probes70, probes32 = ([BC.probes(c, q, 2) for c in cases] for q in (17, 70, 32))
        starts = _starts(boxes3)
        pick = lambda rows: [rows[b] for b in live]                 # noqa: E731
        got = _raw_calls(native, bt, probes17, probes70, probes32, starts, boxes3, scalars)
        ref = _raw_calls(native, two, pick(probes17), pick(probes70), pick(probes32), pick(starts), pick(boxes3), pick(scalars))
        lines = []
        for name, (arrays, status) in got.items():
            want = NOT_PD if name.startswith("optimise") else ERR_ARG
            if status is not None:
                assert list(status) == [OK, want, OK], (name, status)
                assert (ref[name][1] == OK).all(), name
            for a, r in zip(arrays, ref[name][0]):
                assert _untouched(a[1]), name
                for i, b in enumerate(live):
                    assert a[b].tobytes() == r[i].tobytes(), (name, b)
                    assert not _untouched(a[b]), (name, b)
            lines.append("  %-20s %s" % (name, "-" if status is None else list(status)))
        # extend and truncate: the dead run takes no part, the others as in the batch of two
        pts = [BC.new_points(c, 3, b) for b, c in enumerate(cases)]
        Xp, yp = [x for x, _ in pts], np.stack([y for _, y in pts])
        for p, values in ((1, True), (3, False)):
            new_n, status = bt.gp_extend([x[:p] for x in Xp], yp[:, :p] if values else None)
            assert new_n == n + p and list(status) == [OK, ERR_ARG, OK], (p, status)
            _, status2 = two.gp_extend([Xp[b][:p] for b in live], yp[list(live), :p] if values else None)
            assert (status2 == OK).all()
            for i, b in enumerate(live):
                assert _state_bytes(_raw_state(native, bt.ctx[b])) == _state_bytes(_raw_state(native, two.ctx[i])), (p, b)
            _refused(native, lambda: bt.ctx[1].gp_state())
            tst = _filled(3, np.int32)
            bt._chk(native.LIB.pcabo_batch_gp_truncate(bt._h, n, native._ptr(tst)))
            assert bt._follow_n() == n and two.gp_truncate() == n
            lines.append("  extend +%d / truncate  %s / %s" % (p, list(status), list(tst)))
            assert list(tst) == [OK, ERR_ARG, OK], tst
            _refused(native, lambda: bt.ctx[1].gp_state())
        for i, b in enumerate(live):
            assert _state_bytes(_raw_state(native, bt.ctx[b])) == _alone(native, single, cases[b], "ucb", QS[-1])["bytes"], b
        # the lock-step fit: the dead run reports its failure, the others end on the bytes of their own fits
        bt.gp_condition_begin(np.stack([c.Z for c in cases]), np.stack([c.y for c in cases]), gp_noise=0.0)
        fits = bt.gp_fit()
        assert fits[1]["status"] == NOT_PD and fits[0]["status"] == OK and fits[2]["status"] == OK, [f["status"] for f in fits]
        lines.append("  %-20s %s" % ("gp_fit", [f["status"] for f in fits]))
        for b in live:
            own = single.gp_fit(cases[b].y, Z=cases[b].Z)
            assert own["theta"].tobytes() == fits[b]["theta"].tobytes() and own["loss"] == fits[b]["loss"], b
            assert _state_bytes(_raw_state(native, bt.ctx[b])) == _state_bytes(_raw_state(native, single)), b
        _refused(native, lambda: bt.ctx[1].gp_state())
        # all three on plain data in the same batch: the bytes of a fresh batch
        clean = [BC.plain(0), BC.plain(1), BC.plain(2)]
        fresh = native.Batch(3, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q, device_lbfgsb=1)
        try:
            used = _condition_and_score(native, bt, clean, "log_ei", 70)
            new = _condition_and_score(native, fresh, clean, "log_ei", 70)
            assert (used[1] == OK).all() and (new[1] == OK).all() and used[0].tobytes() == new[0].tobytes()
            probes = [BC.probes(c, 17, 2) for c in clean]
            assert _model_bytes_batch(native, bt, probes) == _model_bytes_batch(native, fresh, probes)
            for b, c in enumerate(clean):
                assert _state_bytes(_raw_state(native, bt.ctx[b])) == _alone(native, single, c, "log_ei", 70)["bytes"], b
        finally:
            fresh.close()
    finally:
        bt.close()
        two.close()
    with capsys.disabled():
        print("\na run without a GP (run 1 of 3), status per call\n" + "\n".join(lines))


def test_a_dead_run_in_the_oversubscribed_batch(native, single):
    """B = 86 (the k_chol_lookn form), `dead` at index 7: status -2 for it alone, its values left alone, every other run's state and
    values the bytes of its own context."""
    cases = [BC.plain(s) for s in range(BIG_B)]
    cases[7] = BC.dead(7)
    bt = native.Batch(BIG_B, max_n=BC.N, max_d=MAX_D, max_q=MAX_Q)
    try:
        for acq, q in (("log_ei", 70), ("ucb", 16)):
            codes = [_scalar(native, c, acq) for c in cases]
            bt.gp_condition_begin(np.stack([c.Z for c in cases]), np.stack([c.y for c in cases]), gp_noise=0.0)
            buf, _ = _packed(bt, [BC.probes(c, q) for c in cases])
            val, status, bf = _filled((BIG_B, q)), _filled(BIG_B, np.int32), np.array([s for _, s in codes], dtype=np.float64)
            bt._chk(native.LIB.pcabo_batch_gp_condition_end_eval(bt._h, native._ptr(buf), q, native._ptr(bf), 0, codes[0][0],
                                                                 native._ptr(val), native._ptr(status)))
            assert status[7] == NOT_PD and (np.delete(status, 7) == OK).all(), status
            assert _untouched(val[7])
            _refused(native, lambda: bt.ctx[7].gp_state())
            for b, case in enumerate(cases):
                if b != 7:
                    one = _alone(native, single, case, acq, q)
                    assert _state_bytes(_raw_state(native, bt.ctx[b])) == one["bytes"] and val[b].tobytes() == one["val"], (acq, q, b)
        SEEN.append(("E B86 dead", 7, int(status[7])))
    finally:
        bt.close()


# ---- F. the lock-step likelihood's redo ------------------------------------------------------------------------------------------------
def test_the_lockstep_likelihood_redoes_a_run_alone(native, single):
    """Batch.gp_mll with theta = (1e-300, 0, 0) for `retry` in the middle (inside the domain s2 > 0; 1 + 1e-300 == 1 and softplus(0)
    = ln 2, so its K is the K of the plain conditioning, which leaves rung 0) and an ordinary theta for the others: loss, gradient
    and status are the bytes of Context.gp_mll on each run alone, every member's state those of that context, and the middle run's
    rung is > 0 - the round's factorisation failed for it and mll_attempts redid it alone."""
    cases = [BC.plain(0), BC.retry(), BC.plain(2)]
    thetas = np.array([[0.01, 0.1, 0.2], [1e-300, 0.0, 0.0], [0.02, -0.1, -0.3]])
    bt = native.Batch(3, max_n=MAX_N, max_d=MAX_D, max_q=MAX_Q)
    try:
        bt.gp_condition_begin(np.stack([c.Z for c in cases]), np.stack([c.y for c in cases]), gp_noise=0.0)
        res = bt.gp_mll(thetas)
        assert [r["status"] for r in res] == [OK, OK, OK]
        for b, case in enumerate(cases):
            own = single.gp_mll(case.y, thetas[b], Z=case.Z)
            assert np.float64(own["loss"]).tobytes() == np.float64(res[b]["loss"]).tobytes(), b
            assert own["grad"].tobytes() == res[b]["grad"].tobytes(), b
            st = _raw_state(native, bt.ctx[b])
            assert _state_bytes(st) == _state_bytes(_raw_state(native, single)), b
            rung = _rung(st, bt.ctx[b].gram())
            assert rung == _rung(_raw_state(native, single), single.gram()) and (rung > 0.0) == (b == 1), (b, rung)
            if b == 1:
                SEEN.append(("F lock-step likelihood, climbs", 1, rung))
    finally:
        bt.close()


# ---- G. the driver ---------------------------------------------------------------------------------------------------------------------
def test_the_driver_parks_a_run_whose_conditioning_fails(native, capsys):
    """Three seeded BatchedPCABO runs (f15, d = 5, budget 40, 20 DoE points).  After iteration 5 every coordinate of every stored
    point of run 1 is overwritten with a constant in the array the device reads (the module docstring says why one coordinate is not
    enough for either batched class).  The next iteration's scoring reports -2 for it: pcabo/batchrun.py parks it with its "GP
    conditioning failed" message, and runs 0 and 2 finish with the points and values of a batch of those two alone."""
    from pcabo.batchrun import BatchedPCABO
    insts, dim, budget, n_doe = [0, 1, 2], 5, 40, 20
    seeds = [15000 + 10 * dim + i for i in insts]
    r = BatchedPCABO([BBOBProblem(15, i, dim) for i in insts], seeds, budget, n_doe)
    r.start()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for it in range(budget - n_doe):
            if it == 5:
                assert r.n == n_doe + 5 and r.failed == [None] * 3
                r._X[1, : r.n] = 0.5
            r.iteration()
            if it == 5:
                assert r.failed[1] == (n_doe + 5, "GP conditioning failed (K not positive definite)"), r.failed
    r.finish()
    assert r.failed[0] is None and r.failed[2] is None and len(r.f_evals[1]) == n_doe + 5
    assert any("GP conditioning failed" in str(w.message) and "run 1" in str(w.message) for w in caught)
    alone = BatchedPCABO([BBOBProblem(15, i, dim) for i in (0, 2)], [seeds[0], seeds[2]], budget, n_doe)
    alone.run()
    for i, b in enumerate((0, 2)):
        assert len(r.f_evals[b]) == budget
        assert np.vstack(r.x_evals[b]).tobytes() == np.vstack(alone.x_evals[i]).tobytes(), b
        assert np.array(r.f_evals[b]).tobytes() == np.array(alone.f_evals[i]).tobytes(), b
    SEEN.append(("G driver, parked", 1, NOT_PD))
    with capsys.disabled():
        print("\nrare paths of a batch: what every case saw (rung of the run that climbs, status of the run that ends without a GP)")
        for what, run, seen in SEEN:
            print("  %-44s run %-3d %s" % (what, run, "status %d" % seen if isinstance(seen, int) else "rung %g" % seen))
