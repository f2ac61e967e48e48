"""pcabo.acqopt.propose - q candidates per iteration, one after the other on a model that takes every pending point in - against a
scripted numpy context: which calls it makes, in which order, with which scalar; what the pending points are believed to be worth;
that whatever was appended is taken back, also when a call raises; what it takes from torch's global generator.  Everything but the
context is real: the Sobol engines, the draws, the Boltzmann pick."""
import hashlib

import numpy as np
import pytest
import torch

from pcabo import _native, acqopt
from pcabo import initializers as init

K, RAW, RESTARTS = 3, 16, 4
BOX = np.array([[-1.0] * K, [2.0] * K])
ACQS = {"EI": _native.ACQ_LOG_EI, "PI": _native.ACQ_PI, "UCB": _native.ACQ_UCB}


def _h(a):
    return hashlib.blake2b(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes(), digest_size=4).hexdigest()


class FakeContext:
    """The calls of `_native.Context` the proposal loop makes, answered by cheap numpy; `raises`: {(call, how many calls of that
    name went before): exception}; `failed`: the optimize_acqf calls (by number) that ask for botorch's retry."""

    def __init__(self, n=7, means=(), raises=None, failed=()):
        self.n = self.n_base = n
        self.k = K
        self.means, self.raises, self.failed = list(means), dict(raises or {}), set(failed)
        self.log, self.count = [], {}

    def _enter(self, name, *args):
        i = self.count.get(name, 0)
        self.count[name] = i + 1
        self.log.append((name,) + args)
        if (name, i) in self.raises:
            raise self.raises[(name, i)]
        return i

    def _values(self, X, acq):
        v = -np.mean((np.asarray(X, dtype=np.float64) - 0.25 - 0.01 * self.n) ** 2, axis=-1)
        return np.exp(v) if acq == _native.ACQ_PI else v

    def acq_eval(self, Xq, best_f, maximize=False, acq=0, grad=True):
        assert not grad
        self._enter("acq_eval", self.n, _h(Xq), float(best_f), bool(maximize), int(acq))
        return self._values(Xq, acq)

    def optimize_acqf(self, ics, bounds, best_f, maximize=False, acq=0, batch_limit=5, maxiter=200):
        i = self._enter("optimize_acqf", self.n, _h(ics), _h(bounds), float(best_f), bool(maximize), int(acq), batch_limit, maxiter)
        cand = np.clip(0.9 * np.asarray(ics) + 0.01 * (self.n + 1), bounds[0], bounds[1])
        return cand, self._values(cand, acq), np.array([[3, 4, 0, 1]], dtype=np.int32), i in self.failed

    def gp_posterior(self, Xq, observation_noise=False, covariance=False):
        i = self._enter("gp_posterior", self.n, _h(Xq), bool(observation_noise))
        return {"mean": np.array([self.means[i]]), "variance": np.array([0.5])}

    def gp_extend(self, Zp, y=None):
        self._enter("gp_extend", self.n, _h(Zp), None if y is None else tuple(float(v) for v in y))
        self.n += 1
        return self.n

    def gp_truncate(self, n0=None):
        n0 = self.n_base if n0 is None else n0
        self._enter("gp_truncate", self.n, n0)
        assert self.n_base <= n0 <= self.n
        self.n = n0
        return n0


def _propose(ctx, q_eff, acq="EI", s0=5.0, maximize=False, strategy="kriging_believer", f_evals=None, seed=3, **kw):
    torch.manual_seed(seed)
    return acqopt.propose(ctx, BOX, s0, maximize, ACQS[acq], RESTARTS, RAW, 5, 200, q_eff=q_eff, strategy=strategy,
                          f_evals=f_evals, **kw)


def _names(ctx):
    return [entry[0] for entry in ctx.log]


def _scalars(ctx):
    return [entry[4] for entry in ctx.log if entry[0] == "optimize_acqf"]


def test_call_order_of_three_proposals():
    ctx = FakeContext(means=[4.0, 4.5])
    trace = {}
    Z, infos = _propose(ctx, 3, trace=trace)
    assert _names(ctx) == ["acq_eval", "optimize_acqf", "gp_posterior", "gp_extend", "acq_eval", "optimize_acqf", "gp_posterior",
                           "gp_extend", "acq_eval", "optimize_acqf", "gp_truncate"]
    assert Z.shape == (3, K) and len(infos) == 3 and ctx.n == ctx.n_base == 7
    assert [e[1] for e in ctx.log] == [7, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9]             # the n every call saw
    assert ctx.log[-1] == ("gp_truncate", 9, 7)
    post = [e for e in ctx.log if e[0] == "gp_posterior"]
    ext = [e for e in ctx.log if e[0] == "gp_extend"]
    assert [e[2] for e in post] == [_h(Z[0]), _h(Z[1])] == [e[2] for e in ext]      # believed and appended at the candidate before
    assert all(e[3] is False for e in post) and all(e[3] is None for e in ext)      # no observation noise; believer mode
    # the scoring of a proposal and its optimiser take the same scalar
    assert [e[3] for e in ctx.log if e[0] == "acq_eval"] == _scalars(ctx) == [5.0, 4.0, 4.0]
    # proposal 0 under today's keys, the later ones in "proposals" with what they believed and the scalar they took
    assert {"raw_vals", "ic_idx", "ics", "cands", "vals", "chosen", "info", "k"} <= set(trace)
    assert [(p["best_f"], p["believed"]) for p in trace["proposals"]] == [(4.0, 4.0), (4.0, 4.5)]
    for j, p in enumerate(trace["proposals"]):
        assert {"raw_vals", "ic_idx", "ics", "cands", "vals", "chosen", "info", "k", "best_f", "believed"} == set(p)
        assert np.array_equal(p["cands"][p["chosen"]], Z[j + 1])


@pytest.mark.parametrize("acq,maximize,means,expected", [
    ("EI", False, [4.0, 4.5, 3.0], [5.0, 4.0, 4.0, 3.0]), ("EI", True, [4.0, 6.5, 6.0], [5.0, 5.0, 6.5, 6.5]),
    ("PI", False, [6.0, 4.5, 4.75], [5.0, 5.0, 4.5, 4.5]), ("PI", True, [5.5, 5.25, 7.0], [5.0, 5.5, 5.5, 7.0]),
    ("UCB", False, [4.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]), ("UCB", True, [6.0, 7.0, 8.0], [5.0, 5.0, 5.0, 5.0])])
def test_the_scalar_moves_with_the_believed_value(acq, maximize, means, expected):
    ctx = FakeContext(means=means)
    _propose(ctx, 4, acq=acq, maximize=maximize)
    assert _scalars(ctx) == expected
    assert all(e[5] is maximize and e[6] == ACQS[acq] for e in ctx.log if e[0] == "optimize_acqf")


@pytest.mark.parametrize("strategy,lie", [("constant_liar_min", -2.0), ("constant_liar_mean", 1.5), ("constant_liar_max", 7.0)])
@pytest.mark.parametrize("maximize", [False, True])
def test_the_three_liars(strategy, lie, maximize):
    ctx = FakeContext()
    trace = {}
    _propose(ctx, 3, s0=1.0, maximize=maximize, strategy=strategy, f_evals=[7.0, -2.0, 0.0, 1.0], trace=trace)
    assert "gp_posterior" not in _names(ctx)
    assert [e[3] for e in ctx.log if e[0] == "gp_extend"] == [(lie,), (lie,)]
    s1 = max(1.0, lie) if maximize else min(1.0, lie)
    assert _scalars(ctx) == [1.0, s1, s1]
    assert [p["believed"] for p in trace["proposals"]] == [lie, lie]


def test_unknown_strategy():
    with pytest.raises(ValueError, match="q_strategy"):
        _propose(FakeContext(), 2, strategy="thompson")


@pytest.mark.parametrize("call,index,appended", [("optimize_acqf", 1, 1), ("optimize_acqf", 2, 2), ("gp_extend", 1, 1),
                                                 ("gp_posterior", 1, 1), ("acq_eval", 2, 2)])
def test_taken_back_when_something_raises(call, index, appended):
    ctx = FakeContext(means=[4.0, 4.5], raises={(call, index): _native.PcaboError(-2, "scripted")})
    with pytest.raises(_native.PcaboError, match="scripted"):
        _propose(ctx, 3)
    assert ctx.log[-1] == ("gp_truncate", 7 + appended, 7) and ctx.n == 7
    assert _names(ctx).count("gp_truncate") == 1


@pytest.mark.parametrize("call", ["optimize_acqf", "gp_extend", "gp_posterior"])
def test_nothing_to_take_back_before_the_first_point_is_in(call):
    ctx = FakeContext(means=[4.0], raises={(call, 0): _native.PcaboError(-2, "scripted")})
    with pytest.raises(_native.PcaboError):
        _propose(ctx, 3)
    assert "gp_truncate" not in _names(ctx) and ctx.n == 7


def _engine_draws(seed, q_eff):
    """Where torch's global generator stands after q_eff fresh engines and nothing else (the picks below are deterministic)."""
    torch.manual_seed(seed)
    for _ in range(q_eff):
        init.scrambled_sobol_engine(K)
    return torch.get_rng_state()


@pytest.mark.parametrize("q_eff", [1, 2, 3])
def test_one_engine_per_proposal_from_the_global_generator(q_eff):
    ctx = FakeContext(means=[4.0, 4.5])
    torch.manual_seed(11)
    acqopt.propose(ctx, BOX, 5.0, False, ACQS["EI"], RAW, RAW, q_eff=q_eff)        # (as many restarts as raw samples: no multinomial)
    assert torch.equal(torch.get_rng_state(), _engine_draws(11, q_eff))
    assert _names(ctx).count("optimize_acqf") == q_eff


def test_a_retry_draws_and_scores_afresh_on_the_extended_model():
    ctx = FakeContext(means=[4.0], failed={1})
    trace = {}
    torch.manual_seed(11)
    with pytest.warns(RuntimeWarning, match="trying again"):
        Z, infos = acqopt.propose(ctx, BOX, 5.0, False, ACQS["EI"], RAW, RAW, q_eff=2, trace=trace)
    assert _names(ctx) == ["acq_eval", "optimize_acqf", "gp_posterior", "gp_extend", "acq_eval", "optimize_acqf", "acq_eval",
                           "optimize_acqf", "gp_truncate"]
    assert [e[1] for e in ctx.log[4:8]] == [8, 8, 8, 8] and trace["proposals"][0]["retried"] is True and "retried" not in trace
    assert torch.equal(torch.get_rng_state(), _engine_draws(11, 3)) and len(infos) == 2


def test_q1_makes_the_calls_of_optimize_acqf():
    """One proposal: nothing but optimize_acqf, with what the caller prepared handed through."""
    def run(fn):
        ctx, trace, called = FakeContext(), {}, []
        torch.manual_seed(5)
        engine = init.scrambled_sobol_engine(K)
        raw = init.draw_sobol(BOX, RAW, engine)
        out = fn(ctx, raw, ctx._values(raw, 0) + 1.0, trace, lambda: called.append(len(ctx.log)))
        return ctx.log, trace, called, torch.get_rng_state(), out

    log_a, tr_a, called_a, rng_a, (z, cand, vals, info) = run(lambda ctx, raw, rv, tr, hook: acqopt.optimize_acqf(
        ctx, BOX, 5.0, False, 0, RESTARTS, RAW, 5, 200, raw=raw, raw_vals=rv, trace=tr, before_lbfgsb=hook))
    log_b, tr_b, called_b, rng_b, (Z, infos) = run(lambda ctx, raw, rv, tr, hook: acqopt.propose(
        ctx, BOX, 5.0, False, 0, RESTARTS, RAW, 5, 200, q_eff=1, f_evals=[1.0], raw=raw, raw_vals=rv, trace=tr, before_lbfgsb=hook))
    assert log_a == log_b and [e[0] for e in log_b] == ["optimize_acqf"] and called_a == called_b == [0]
    assert torch.equal(rng_a, rng_b) and Z.tobytes() == z.tobytes() and len(infos) == 1 and infos[0] is not None
    assert set(tr_a) == set(tr_b) and "proposals" not in tr_b
    assert all(np.array_equal(tr_a[key], tr_b[key]) for key in tr_a)


def test_helpers():
    assert acqopt.liar_value("constant_liar_mean", [1, 2, 6]) == 3.0
    assert acqopt.moved_scalar(2.0, 1.0, False, ACQS["PI"]) == 1.0 and acqopt.moved_scalar(2.0, 1.0, True, ACQS["EI"]) == 2.0
    assert acqopt.moved_scalar(2.0, 1.0, False, ACQS["UCB"]) == 2.0


@pytest.mark.parametrize("evaluated,expected", [(6, 3), (10, 3), (11, 2), (12, 1)])
def test_the_class_hands_propose_what_the_budget_leaves(monkeypatch, evaluated, expected):
    """Vanilla_BO(budget=13, q=3) over the scripted context: the iteration at n evaluated points proposes min(q, 13 - n)."""
    from Algorithms import Vanilla_BO
    from Algorithms.BayesianOptimization.DeviceBayesianOptimizer import LogExpectedImprovement
    monkeypatch.setenv("SMOKE_TEST", "1")                                # 32 raw samples, 2 restarts
    opt = Vanilla_BO(budget=13, n_DoE=6, q=3)
    ctx = FakeContext(n=evaluated, means=[4.0, 4.5])
    ctx.gp_wait_eval = lambda raw, s, maximize, acq: ctx.acq_eval(raw, s, maximize, acq, grad=False)
    opt._ctx, opt.dimension = ctx, K
    opt._Vanilla_BO__box = BOX
    opt.f_evals.extend([1.0] * evaluated)
    opt.acquisition_function = LogExpectedImprovement(best_f=5.0, maximize=False)
    torch.manual_seed(2)
    Z = opt.optimize_acqf_and_get_observation()
    assert Z.shape == (expected, K) and _names(ctx).count("optimize_acqf") == expected == len(opt.lbfgsb_info)
    assert _names(ctx).count("gp_extend") == expected - 1 and len(opt.timing_logs["optimize_acqf"]) == 1
    assert ctx.n == evaluated and (_names(ctx)[-1] == "gp_truncate") == (expected > 1)
