"""Scoring of the raw samples, initial pick and optimiser of a single run in one native call (pcabo_propose_acqf,
Context.propose_acqf; the keyword one_call= of PCA_BO / Vanilla_BO, on by default) against the three calls with torch's pick
between them: the same bytes everywhere and the same state of torch's global generator afterwards.

Whole runs: d = 5, n_DoE = 8, budget = 20 - twelve iterations per run, stepped so that the generator can be read before the run
puts the caller's states back.  Direct calls: n = 8 points in k = 2 dimensions, a conditioning in flight or ended, few and many raw
samples (the small path, one 64-sample tile, the 512 of a BO iteration), scores without spread, the jitter ladder (the case of
tests/test_gpu_score_split.py, whose Gram matrix cannot be factored at rung 0), the refusals with their texts, and the evaluation
paths of the optimiser that a keyword or the profiling mode selects."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ERR_ARG = -1
TRACE_KEYS = ("raw_vals", "ic_idx", "ics", "cands", "vals", "chosen")
ITERATIONS = 12


def _run(native, monkeypatch, cls, acq_kwargs, one_call):
    from Algorithms import PCA_BO, Vanilla_BO
    from pcabo.bbob import BBOBProblem
    calls = []
    real = native.Context.propose_acqf
    monkeypatch.setattr(native.Context, "propose_acqf", lambda self, *a, **kw: (calls.append(1), real(self, *a, **kw))[1])
    opt = {"pca": PCA_BO, "vanilla": Vanilla_BO}[cls](budget=20, n_DoE=8, random_seed=11, record_trace=True, one_call=one_call,
                                                      **acq_kwargs)
    problem = BBOBProblem(15, 1, 5)
    try:
        opt._start(problem)
        for _ in range(ITERATIONS):
            opt._bo_iteration(problem)
        state = torch.get_rng_state().numpy().copy()
    finally:
        opt._finish()
    return opt, state, len(calls)


def _same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("acq", ["EI", "UCB"])
@pytest.mark.parametrize("cls", ["pca", "vanilla"])
def test_whole_runs_are_the_same_with_one_call_and_with_three(native, monkeypatch, cls, acq):
    kw = {"acquisition_function": acq, **({"ucb_beta": 2.0} if acq == "UCB" else {})}
    on, state_on, calls_on = _run(native, monkeypatch, cls, kw, True)
    off, state_off, calls_off = _run(native, monkeypatch, cls, kw, False)
    assert (calls_on, calls_off) == (ITERATIONS, 0)
    assert len(on.f_evals) == len(off.f_evals) == 20
    assert _same_bytes(np.vstack(on.x_evals), np.vstack(off.x_evals)) and _same_bytes(on.f_evals, off.f_evals)
    assert len(on.lbfgsb_info) == len(off.lbfgsb_info) == ITERATIONS
    for it in range(ITERATIONS):
        assert _same_bytes(on.lbfgsb_info[it], off.lbfgsb_info[it]), it
        for key in TRACE_KEYS:
            assert _same_bytes(on.trace[it][key], off.trace[it][key]), (it, key)
        assert _same_bytes(on.trace[it]["info"], off.trace[it]["info"]), it
    assert np.array_equal(state_on, state_off)
    assert set(on.phase_breakdown) == set(off.phase_breakdown) == {"sobol", "raw_eval", "init_pick", "lbfgsb"}
    assert all(v > 0.0 for key, v in on.phase_breakdown.items() if key != "sobol" or cls == "pca")


@pytest.mark.parametrize("cls", ["pca", "vanilla"])
def test_pi_keeps_the_three_calls(native, monkeypatch, cls):
    kw = {"acquisition_function": "PI"}
    on, state_on, calls_on = _run(native, monkeypatch, cls, kw, True)
    off, state_off, calls_off = _run(native, monkeypatch, cls, kw, False)
    assert (calls_on, calls_off) == (0, 0)
    assert _same_bytes(np.vstack(on.x_evals), np.vstack(off.x_evals)) and _same_bytes(on.f_evals, off.f_evals)
    assert np.array_equal(state_on, state_off)


# ---- direct calls ----------------------------------------------------------------------------------------------------------------
N, K, RESTARTS = 8, 2, 4


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=256, max_d=8, max_q=512)
    yield c
    c.close()


def _design(n_raw, seed=3):
    rng = np.random.default_rng([seed, n_raw])
    Z = rng.uniform(-2.0, 2.0, (N, K))
    y = rng.normal(size=N) * 30.0 + 100.0
    return Z, y, rng


def _three_calls(native, ctx, Z, y, raw, nr, scalar, code, pending, seed, noise=None, batch_limit=2):
    from pcabo import initializers as I
    extra = {} if noise is None else {"noise": noise}
    torch.manual_seed(seed)
    ctx.gp_condition(y, Z=Z, wait=not pending, **extra)
    bounds = ctx.acq_bounds()
    vals = ctx.gp_wait_eval(raw, scalar, acq=code) if pending else ctx.acq_eval(raw, scalar, acq=code, grad=False)
    idx = I.initialize_q_batch(vals, nr)
    ics = raw[idx]
    cand, v, info, failed = ctx.optimize_acqf(ics, bounds, scalar, acq=code, batch_limit=batch_limit)
    return {"raw_vals": vals, "ic_idx": np.asarray(idx), "ics": ics, "cand": cand, "vals": v, "info": info, "failed": failed,
            "state": torch.get_rng_state().numpy().copy()}


def _one_call(native, ctx, Z, y, raw, nr, scalar, code, pending, seed, noise=None, batch_limit=2, **kw):
    extra = {} if noise is None else {"noise": noise}
    torch.manual_seed(seed)
    blob = torch.get_rng_state().numpy()
    ctx.gp_condition(y, Z=Z, wait=not pending, **extra)
    bounds = ctx.acq_bounds()
    r = ctx.propose_acqf(raw, blob, nr, bounds, scalar, acq=code, batch_limit=batch_limit, **kw)
    r["state"] = blob
    return r


def _assert_same(one, three, what):
    assert one["picked"], what
    for key in ("raw_vals", "ic_idx", "ics", "cand", "vals", "info", "state"):
        assert _same_bytes(one[key], three[key]), (what, key)
    assert one["failed"] == three["failed"], what
    assert one["phase_seconds"].shape == (3,) and (one["phase_seconds"] > 0.0).all(), what


@pytest.mark.parametrize("acq", ["log_ei", "ucb"])
@pytest.mark.parametrize("pending", [True, False])
@pytest.mark.parametrize("n_raw", [10, 64, 512])
def test_one_call_equals_the_three_calls(native, ctx, n_raw, pending, acq):
    Z, y, rng = _design(n_raw)
    raw = rng.uniform(Z.min(0) - 0.3, Z.max(0) + 0.3, (n_raw, K))
    code, scalar = (native.ACQ_LOG_EI, float(y.min())) if acq == "log_ei" else (native.ACQ_UCB, 1.5)
    three = _three_calls(native, ctx, Z, y, raw, RESTARTS, scalar, code, pending, seed=n_raw)
    one = _one_call(native, ctx, Z, y, raw, RESTARTS, scalar, code, pending, seed=n_raw)
    _assert_same(one, three, (n_raw, pending, acq))
    asleep = _one_call(native, ctx, Z, y, raw, RESTARTS, scalar, code, pending, seed=n_raw, wake=False)
    _assert_same(asleep, three, (n_raw, pending, acq, "helper left asleep"))
    single = _three_calls(native, ctx, Z, y, raw, RESTARTS, scalar, code, pending, seed=n_raw, batch_limit=5)     # one group: no helper
    _assert_same(_one_call(native, ctx, Z, y, raw, RESTARTS, scalar, code, pending, seed=n_raw, batch_limit=5), single, "one group")


@pytest.mark.parametrize("pending", [True, False])
def test_scores_without_spread_are_left_to_the_caller(native, ctx, pending):
    """Two identical raw points: equal scores, nothing picked, the blob untouched, the scores right - and the context is ready for
    the optimiser the caller then starts itself."""
    Z, y, rng = _design(2)
    raw = np.repeat(rng.uniform(-1.0, 1.0, (1, K)), 2, axis=0)
    scalar = float(y.min())
    torch.manual_seed(9)
    start = torch.get_rng_state().numpy().copy()
    r = _one_call(native, ctx, Z, y, raw, 1, scalar, native.ACQ_LOG_EI, pending, seed=9)
    assert not r["picked"] and set(r) == {"raw_vals", "picked", "phase_seconds", "state"}
    assert np.array_equal(r["state"], start)
    want = ctx.acq_eval(raw, scalar, grad=False)
    assert r["raw_vals"].tobytes() == want.tobytes() and want[0] == want[1]
    cand, v, _, _ = ctx.optimize_acqf(raw[:1], ctx.acq_bounds(), scalar)
    assert np.isfinite(cand).all() and np.isfinite(v).all()


def test_one_call_behind_a_jitter_retry(native, ctx):
    from test_gpu_score_split import retry_case, _rung
    Z, y, raw = retry_case()
    scalar = float(y.min())
    three = _three_calls(native, ctx, Z, y, raw, 10, scalar, native.ACQ_LOG_EI, True, seed=4, noise=0.0, batch_limit=5)
    assert _rung(ctx)[0] > 0.0, "the retry case was factored at rung 0: the retry was not exercised"
    one = _one_call(native, ctx, Z, y, raw, 10, scalar, native.ACQ_LOG_EI, True, seed=4, noise=0.0, batch_limit=5)
    assert _rung(ctx)[0] > 0.0
    _assert_same(one, three, "jitter")


def test_other_evaluation_paths_give_the_same_bytes(native):
    """resident=False (PCABO_OPT_RESIDENT 0) and the profiling mode, which takes plain launches and no second stream."""
    Z, y, rng = _design(512, seed=8)
    raw = rng.uniform(Z.min(0) - 0.3, Z.max(0) + 0.3, (512, K))
    scalar = float(y.min())
    got = {}
    for name in ("default", "not_resident", "profiling"):
        c = native.Context(max_n=16, max_d=K, max_q=512)
        try:
            if name == "not_resident":
                c.set_option(native.OPT_RESIDENT, 0)
            if name == "profiling":
                c.set_profiling(True)
            got[name] = _one_call(native, c, Z, y, raw, 10, scalar, native.ACQ_LOG_EI, True, seed=2, batch_limit=5)
            if name == "default":
                three = _three_calls(native, c, Z, y, raw, 10, scalar, native.ACQ_LOG_EI, True, seed=2, batch_limit=5)
        finally:
            c.close()
    for name, r in got.items():
        _assert_same(r, three, name)


def refused(call, text, code=ERR_ARG):
    with pytest.raises(Exception) as e:
        call()
    assert type(e.value).__name__ == "PcaboError", repr(e.value)
    assert e.value.code == code and str(e.value) == "libpcabo error %d: %s" % (code, text), str(e.value)


def test_refusals(native):
    Z, y, rng = _design(16)
    raw = rng.uniform(-2.0, 2.0, (16, K))
    box = np.array([[-2.0] * K, [2.0] * K])
    good = torch.Generator().manual_seed(1).get_state().numpy().copy()
    c = native.Context(max_n=16, max_d=K, max_q=16)
    try:
        c.n, c.d, c.k = N, K, K
        ask = lambda blob=good, nr=4, raw=raw, acq=native.ACQ_LOG_EI, s=0.0: c.propose_acqf(raw, blob.copy(), nr, box, s, acq=acq)  # noqa: E731
        refused(ask, "pcabo_propose_acqf: call pcabo_gp_condition first")                  # a new context
        c.gp_condition(y, Z=Z, wait=False)                                                # in flight: the argument rules
        refused(lambda: ask(raw=np.zeros((17, K))), "pcabo_propose_acqf: bad argument or q beyond context capacity")
        refused(lambda: ask(nr=16), "pcabo_propose_acqf: the pick takes fewer restarts than raw samples, of at least two")
        refused(lambda: ask(acq=native.ACQ_PI), "pcabo_propose_acqf: the pick of PCABO_ACQ_PI (botorch's non-negative variant) is the caller's")
        refused(lambda: ask(acq=7), "pcabo_propose_acqf: unknown acquisition code")
        refused(lambda: ask(acq=native.ACQ_UCB, s=-1.0),
                "pcabo_propose_acqf: PCABO_ACQ_UCB takes kappa = sqrt(beta) in the best_f slot: it must be finite and >= 0")
        past = good.copy()                                                                # left = 624, next = 2: reads state[624]
        past[8:12] = np.frombuffer(np.int32(624).tobytes(), dtype=np.uint8)
        past[16:24] = np.frombuffer(np.uint64(2).tobytes(), dtype=np.uint8)
        refused(lambda: ask(blob=past), "pcabo_propose_acqf: not a state blob of torch's CPU generator")
        with pytest.raises(ValueError):
            c.propose_acqf(raw, good[:100].copy(), 4, box, 0.0)
        assert ask()["picked"]                                                            # ... and the conditioning is still there
        assert ask()["picked"]                                                            # conditioned: goes ahead as well
        refused(lambda: c.gp_wait_eval(raw, 0.0), "pcabo_gp_condition_end_eval: no conditioning in flight")
    finally:
        c.close()
