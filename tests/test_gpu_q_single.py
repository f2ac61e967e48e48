"""q candidates per iteration in a single run on the MI355X (PCA_BO / Vanilla_BO q=..., pcabo.acqopt.propose).

  budget      n_DoE 6, budget 13, q 3 goes 6 -> 9 -> 12 -> 13: the last iteration proposes what the budget leaves.
  taken back  inside the objective the run's context holds the iteration's own points only (n == n_base): the pending points left
              the model before the first of them was observed.
  bits        two runs give the same bytes; a run whose objective is a plain callable (no noise prefetch) gives them too.
  composed    every iteration again through the public Context calls - gp_posterior, gp_extend, acqopt.optimize_acqf, gp_truncate -
              from the traced state of torch's generator: the same candidates bytewise, and the generator ends where the run left it.
              On the extended context the optimiser's values are those Context.acq_eval gives at its candidates (two kernels, two
              summation orders of one fp64 function: 1e-6 relative is far above their distance and far below what a stale n gives).
  moved       s_{j+1} is the better of s_j and the believed value, exactly; the q candidates of an iteration are pairwise distinct;
              log-EI at z_0 on the extended model with the moved incumbent lies below its value on M_0 with s_0.
  q = 1       the keyword at its default changes nothing: the bytes of a run without it, and no "proposals" in the trace.
  64 rows     n_DoE 62, budget 67, q 3: the extended model fills the 64th row inside the proposal loop.
"""
import warnings

import numpy as np
import pytest
import torch

from pcabo import acqopt
from pcabo.bbob import BBOBProblem

pytestmark = pytest.mark.gpu

CASES = [("PCA_BO", {}), ("PCA_BO", {"acq_kernel": "group"}), ("Vanilla_BO", {})]
IDS = ["PCA_BO", "PCA_BO-group", "Vanilla_BO"]
SEED, BOX = 15051, np.array([-5.0, 5.0])


@pytest.fixture(autouse=True)
def _full_sized(monkeypatch):
    monkeypatch.delenv("SMOKE_TEST", raising=False)               # 512 raw samples: the later proposals score through the GEMM


def _cls(name):
    import Algorithms
    return getattr(Algorithms, name)


def _run(cls, problem=None, n_doe=6, budget=13, **kw):
    opt = cls(budget=budget, n_DoE=n_doe, random_seed=SEED, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)           # (botorch's retry warning is not what these tests are about)
        opt(problem=problem if problem is not None else BBOBProblem(15, 0, 5), dim=5, bounds=BOX)
    return opt


def _bytes(opt):
    return np.array(opt.x_evals).tobytes(), np.array(opt.f_evals, dtype=np.float64).tobytes()


def _composing(base):
    """The class with every iteration proposed a second time by hand, through the public calls."""
    class Composing(base):
        def optimize_acqf_and_get_observation(self):
            got = super().optimize_acqf_and_get_observation()
            ctx, acq, cfg, tr = self._ctx, self.acquisition_function, self._torch_config, self.trace[-1]
            after = torch.get_rng_state()
            torch.set_rng_state(tr["torch_state"])
            box = ctx.acq_bounds() if base.__name__ == "PCA_BO" else np.ascontiguousarray(self.bounds.T, dtype=np.float64)
            n0, s, mine, moved = ctx.n, acq.device_scalar, [], []
            assert n0 == ctx.n_base == len(self.f_evals)
            try:
                for j in range(len(got)):
                    z, cand, vals, _ = acqopt.optimize_acqf(ctx, box, s, acq.maximize, acq.acq_code, cfg["NUM_RESTARTS"],
                                                            cfg["RAW_SAMPLES"], 5, 200)
                    again = ctx.acq_eval(cand, s, acq.maximize, acq.acq_code, grad=False)
                    assert np.allclose(again, vals, rtol=1e-6, atol=1e-9), (j, again, vals)
                    mine.append(z)
                    if j == 0:
                        at_z0 = ctx.acq_eval(z, s, acq.maximize, acq.acq_code, grad=False)[0]
                    if j == len(got) - 1:
                        break
                    v = float(ctx.gp_posterior(z)["mean"][0])
                    assert ctx.gp_extend(z) == n0 + j + 1
                    s = min(s, v)
                    moved.append((s, v))
                    if j == 0:                                    # the variance at z_0 is gone and the incumbent moved there
                        assert ctx.acq_eval(mine[0], s, acq.maximize, acq.acq_code, grad=False)[0] < at_z0
            finally:
                ctx.gp_truncate(n0)
            assert np.concatenate(mine).tobytes() == np.asarray(got).tobytes()
            assert torch.equal(torch.get_rng_state(), after)
            for (s_j, v_j), rec in zip(moved, tr.get("proposals", [])):
                assert rec["best_f"] == s_j and rec["believed"] == v_j
            self.composed.append(len(got))
            return got
    return Composing


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_q3_reaches_the_budget_with_the_model_taken_back(name, kw):
    seen = []
    problem = BBOBProblem(15, 0, 5)

    def objective(x):
        ctx = opt.device_context
        seen.append((len(opt.f_evals), ctx.n, ctx.n_base) if ctx is not None else (len(opt.f_evals), 0, 0))
        return problem(x)

    opt = _cls(name)(budget=13, n_DoE=6, random_seed=SEED, q=3, record_trace=True, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        opt(problem=objective, dim=5, bounds=BOX)
    assert len(opt.x_evals) == len(opt.f_evals) == 13 and opt.number_of_function_evaluations == 13
    assert [tr["n"] for tr in opt.trace] == [6, 9, 12]
    assert [len(tr.get("proposals", [])) for tr in opt.trace] == [2, 2, 0]
    assert len(opt.lbfgsb_info) == 7 and len(opt.timing_logs["optimize_acqf"]) == 3
    bo = [s for s in seen if s[1] > 0]                            # (the initial design is evaluated before the context exists)
    assert len(bo) >= 7 - 3                                       # out-of-box candidates of PCA_BO are not evaluated
    for _, n, n_base in bo:
        assert n == n_base and n in (6, 9, 12)
    for tr in opt.trace:
        s, maximize = tr["best_f"], False
        zs = [tr["cands"][tr["chosen"]]] + [p["cands"][p["chosen"]] for p in tr.get("proposals", [])]
        for a in range(len(zs)):
            for b in range(a):
                assert not np.array_equal(zs[a], zs[b])
        for p in tr.get("proposals", []):
            assert p["best_f"] == min(s, p["believed"]) and not maximize
            assert p["chosen"] == int(np.argmax(p["vals"])) and p["raw_vals"].shape == (opt.torch_config["RAW_SAMPLES"],)
            s = p["best_f"]
    # the same run with the in-repo problem (PCA_BO then draws the next iteration's noise ahead, for n + q_eff points) and twice
    plain = [_run(_cls(name), q=3, **kw) for _ in range(2)]
    assert _bytes(plain[0]) == _bytes(plain[1]) == _bytes(opt)


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_composed_through_the_public_calls(name, kw):
    opt = _composing(_cls(name))(budget=13, n_DoE=6, random_seed=SEED, q=3, record_trace=True, **kw)
    opt.composed = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        opt(problem=BBOBProblem(15, 0, 5), dim=5, bounds=BOX)
    assert opt.composed == [3, 3, 1]
    assert _bytes(opt) == _bytes(_run(_cls(name), q=3, **kw))


@pytest.mark.parametrize("strategy", ["constant_liar_min", "constant_liar_mean", "constant_liar_max"])
def test_constant_liar_runs(strategy):
    runs = [_run(_cls("PCA_BO"), q=3, q_strategy=strategy, record_trace=True) for _ in range(2)]
    assert _bytes(runs[0]) == _bytes(runs[1]) and len(runs[0].f_evals) == 13
    pick = {"constant_liar_min": np.min, "constant_liar_mean": np.mean, "constant_liar_max": np.max}[strategy]
    for tr in runs[0].trace:
        lie = float(pick(np.array(runs[0].f_evals[:tr["n"]], dtype=np.float64)))
        assert all(p["believed"] == lie for p in tr.get("proposals", []))
    assert _bytes(runs[0]) != _bytes(_run(_cls("PCA_BO"), q=3))


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_q1_is_the_run_without_the_keyword(name, kw):
    plain, one = _run(_cls(name), record_trace=True, **kw), _run(_cls(name), q=1, record_trace=True, **kw)
    assert _bytes(plain) == _bytes(one) and len(one.f_evals) == 13
    assert all("proposals" not in tr for tr in one.trace) and len(one.lbfgsb_info) == 7
    assert _bytes(one) != _bytes(_run(_cls(name), q=3, **kw))


@pytest.mark.parametrize("name,kw", CASES, ids=IDS)
def test_the_64th_row_inside_the_loop(name, kw):
    seen = []
    problem = BBOBProblem(15, 0, 5)

    def objective(x):
        ctx = opt.device_context
        if ctx is not None and ctx.n:
            seen.append((ctx.n, ctx.n_base))
        return problem(x)

    opt = _cls(name)(budget=67, n_DoE=62, random_seed=SEED, q=3, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        opt(problem=objective, dim=5, bounds=BOX)
    assert len(opt.f_evals) == 67 and len(opt.lbfgsb_info) == 5
    assert all(n == n_base and n in (62, 65) for n, n_base in seen)
    assert _bytes(opt) == _bytes(_run(_cls(name), n_doe=62, budget=67, q=3, **kw))


# ---- semantics: the traced proposals against the extended reference ------------------------------------------------------------------
# Vanilla_BO, whose model inputs are the evaluated points themselves: from a traced q = 3 run the long-double model of every
# iteration is rebuilt on the n observed points with the DEVICE's held transforms (Normalize bounds, Standardize statistics, read
# from the context at M_0) and extended, believer mode, by z_0 .. z_{j-1} (extend_reference.reference_state).  Judged per proposal j:
#   believed   the recorded v_j against the reference's posterior mean of M_j at z_j, in units of s;
#   raw_vals   the recorded values of proposal j's raw samples (64 of them: the GEMM scoring for j >= 1, gp_wait_eval for j = 0)
#              against the reference acquisition on M_j with the scalar s_j as the device takes it (float32, as botorch stores it);
# by the rule of tests/test_gpu_extend.py for its end-to-end comparison, its factors imported from there: every error within ALLOWED x
# the largest error of the plain-fp64 numpy restatement of the same model against the same reference, or within UNITS of the entry's
# first-order unit (acq_reference's for the mean and for log-EI; for UCB value = -mean + kappa sigma the unit is put together from the
# same pieces: dmu + kappa dsigma + 2 eps |value|).  Then what only a moved incumbent gives, on the reference first and on the device
# after it: log-EI at z_0 under (M_1, s_1) lies below its value under (M_0, s_0), and the candidates of an iteration are distinct.
SEM = {}                                                          # acquisition -> (run, {n: (state at M_0, raw samples per proposal)})


def _traced_vanilla(acq_kw):
    key = tuple(sorted(acq_kw.items()))
    if key in SEM:
        return SEM[key]
    from pcabo import initializers
    base = _cls("Vanilla_BO")
    drawn = []
    real = initializers.draw_sobol

    def recording(*a, **kw):
        out = real(*a, **kw)
        drawn.append(np.array(out))
        return out

    class Watched(base):
        def optimize_acqf_and_get_observation(self):
            del drawn[:]
            got = super().optimize_acqf_and_get_observation()
            self.seen[len(self.f_evals)] = (self._ctx.gp_state(), list(drawn))
            return got

    opt = Watched(budget=16, n_DoE=10, random_seed=SEED, q=3, record_trace=True, **acq_kw)
    opt.seen = {}
    opt.torch_config["RAW_SAMPLES"], opt.torch_config["NUM_RESTARTS"] = 64, 4
    initializers.draw_sobol = recording
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            opt(problem=BBOBProblem(15, 0, 5), dim=5, bounds=BOX)
    finally:
        initializers.draw_sobol = real
    SEM[key] = opt
    return opt


@pytest.mark.parametrize("acq_kw", [{}, {"acquisition_function": "UCB", "ucb_beta": 2.0}], ids=["EI", "UCB"])
def test_proposals_against_the_extended_reference(native, acq_kw):
    import acq_reference as AR
    import extend_reference as ER
    from types import SimpleNamespace
    from test_gpu_extend import _within
    from wpca_reference import EPS, f64, hp
    from Algorithms.BayesianOptimization.DeviceBayesianOptimizer import LENGTHSCALE, NOISE
    ucb = bool(acq_kw)
    opt = _traced_vanilla(acq_kw)
    assert [tr["n"] for tr in opt.trace] == [10, 13] and len(opt.f_evals) == 16
    X, f = np.array(opt.x_evals, dtype=np.float64), np.array(opt.f_evals, dtype=np.float64)
    worst, bad = {}, []

    def judge(name, dev_err, yard_err, unit):
        ok, d, y = _within(dev_err, yard_err, unit)
        prev = worst.get(name, (0.0, 0.0, 0.0))
        worst[name] = max(prev, (d / y if y > 0.0 else 0.0, d, y))
        print("  %s: device %.3e restatement %.3e" % (name, d, y))
        if not ok:
            bad.append((name, d, y))

    for tr in opt.trace:
        n = tr["n"]
        st0, raws = opt.seen[n]
        records = [tr] + tr["proposals"]
        assert len(raws) == len(records) == 3 and not any(r.get("retried") for r in records)       # (the seed: no retry in this run)
        case = SimpleNamespace(Z=np.ascontiguousarray(X[:n]), y=f[:n].copy(), n=n, k=5, lengthscale=LENGTHSCALE, noise=NOISE,
                               kernel="matern", norm_bounds=st0["norm_bounds"], gen="run", hyper="default", id="run-n%d" % n)
        held = (st0["norm_bounds"], float(st0["y_mean"]), float(st0["y_std"]))
        s_y = held[2]
        zs = np.vstack([r["cands"][r["chosen"]] for r in records])
        scal = [opt.acquisition_function.kappa if ucb else tr["best_f"]] + [p["best_f"] for p in tr["proposals"]]
        refs = []
        for j, rec in enumerate(records):
            ref, res = ER.reference_state(case, zs[:j], None, held), ER.restated_state(case, zs[:j], None, held)
            refs.append(ref)
            ast = ER.acq_state(ref.case)
            s_dev = float(np.float32(scal[j]))                    # Python floats all the way: botorch stores them as float32
            lin = AR.linear(ast, ref.gs, raws[j])
            what = "n%d p%d" % (n, j)
            if ucb:
                rp, sp = ER.posterior(ref, raws[j]), ER.posterior(res, raws[j])
                value = lambda post: -post["mean"] + s_dev * np.sqrt(np.maximum(post["variance"], AR.FLOOR))
                sig = np.sqrt(np.maximum(f64(rp["variance"]), AR.FLOOR))
                dmu = s_y * lin.dmus + 2.0 * EPS * (abs(held[1]) + np.abs(s_y * f64(lin.mus)))
                dvar = s_y * s_y * (lin.dvv + EPS * (1.0 + 3.0 * np.abs(f64(1 - lin.vv))))
                unit = dmu + s_dev * (dvar / (2.0 * sig) + EPS * sig) + 2.0 * EPS * np.abs(f64(value(rp)))
                judge(what + " raw_vals", hp(rec["raw_vals"]) - value(rp), hp(value(sp)) - value(rp), unit)
            else:
                sc = AR.scalars(lin, s_dev, 0, AR.LOG_EI)
                rv, _ = AR.restate(ast, res.gs, raws[j], s_dev, 0, AR.LOG_EI)
                judge(what + " raw_vals", hp(rec["raw_vals"]) - sc.value, hp(rv) - sc.value, sc.u_value)
            assert rec["chosen"] == int(np.argmax(rec["vals"]))
            if j + 1 < len(records):
                nxt = records[j + 1]
                z = zs[j:j + 1]
                lz = AR.linear(ast, ref.gs, z)
                u_mean = lz.dmus + 2.0 * EPS * (abs(held[1]) / s_y + np.abs(f64(lz.mus)))
                want, rest = ER.posterior(ref, z)["mean"], ER.posterior(res, z)["mean"]
                judge(what + " believed", (hp(np.array([nxt["believed"]])) - want) / s_y, (hp(rest) - want) / s_y, u_mean)
                assert nxt["best_f"] == (scal[j] if ucb else min(scal[j], nxt["believed"]))
        for a in range(3):
            for b in range(a):
                assert not np.array_equal(zs[a], zs[b])
        if not ucb:
            # a loop that forgets to move the incumbent proposes z_0 again: on the reference first, then on the device
            s0, s1 = float(np.float32(scal[0])), float(np.float32(scal[1]))
            at = lambda ref, s: float(AR.scalars(AR.linear(ER.acq_state(ref.case), ref.gs, zs[:1]), s, 0, AR.LOG_EI).value[0])
            assert at(refs[1], s1) < at(refs[0], s0), n
            c = native.Context(max_n=32, max_d=5, max_q=16)
            try:
                ident = np.vstack([np.zeros(5), np.ones(5)])
                c.gp_condition(f[:n], Z=X[:n], norm_bounds=ident)
                c.match_best_f_dtype(scal[0])
                before = c.acq_eval(zs[:1], scal[0], grad=False)[0]
                c.gp_extend(zs[:1])
                assert c.acq_eval(zs[:1], scal[1], grad=False)[0] < before, n
            finally:
                c.close()
    print("  worst device / restatement:", {k: "%.2f (%.2e / %.2e)" % v for k, v in worst.items()})
    assert not bad, bad
