"""The `q` / `q_strategy` keywords where a user meets them, without a device: PCA_BO and Vanilla_BO, the lock-step batch classes, the
experiment runner and the command line.  Before the keywords existed `q=3` travelled on to AbstractAlgorithm, which ignores what it does not know."""
import importlib.util
import os

import pytest

from Algorithms import ExperimentRunner, PCA_BO, Vanilla_BO
from pcabo import acqopt

both = pytest.mark.parametrize("cls", [PCA_BO, Vanilla_BO])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@both
def test_defaults(cls):
    opt = cls(budget=10)
    assert (opt._q, opt._q_strategy) == (1, "kriging_believer")
    assert acqopt.Q_STRATEGIES == ("kriging_believer", "constant_liar_min", "constant_liar_mean", "constant_liar_max")


@both
@pytest.mark.parametrize("strategy", acqopt.Q_STRATEGIES)
def test_accepted(cls, strategy):
    opt = cls(budget=10, q=3, q_strategy=strategy)
    assert (opt._q, opt._q_strategy) == (3, strategy) and type(opt._q) is int


@both
@pytest.mark.parametrize("kwargs", [{"q": 0}, {"q": -1}, {"q": 2.0}, {"q": 2.5}, {"q": "3"}, {"q": True}, {"q": None},
                                    {"q": 2, "q_strategy": "thompson"}, {"q_strategy": "Kriging_Believer"}, {"q_strategy": None}])
def test_constructor_refusals(cls, kwargs):
    with pytest.raises(ValueError, match="q"):
        cls(budget=10, **kwargs)


@both
def test_the_last_iteration_proposes_what_the_budget_leaves(cls):
    opt = cls(budget=13, n_DoE=6, q=3)
    seen = []
    opt.f_evals.extend([0.0] * 6)
    for n in range(6, 13):
        assert len(opt.f_evals) == n
        seen.append(opt._q_eff())
        opt.f_evals.append(0.0)
    assert seen == [3, 3, 3, 3, 3, 2, 1]
    opt = cls(budget=13, n_DoE=6)
    opt.f_evals.extend([0.0] * 6)
    assert opt._q_eff() == 1


def _runner(**kw):
    return ExperimentRunner(algorithms=["pca"], dimensions=[5], problem_ids=[15], num_runs=1, progress=False, **kw)


def test_runner():
    r = _runner()
    assert (r.q, r.q_strategy) == (1, "kriging_believer")
    r = _runner(q=4, q_strategy="constant_liar_min")
    assert (r.q, r.q_strategy) == (4, "constant_liar_min")
    for kw in ({"q": 0}, {"q": 1.5}, {"q": 2, "q_strategy": "x"}, {"q": True}):
        with pytest.raises(ValueError):
            _runner(**kw)
    assert _runner(q=2, batched=4).q == 2


class _Problem:
    class meta_data:
        n_variables = 3

    class bounds:
        lb, ub = [-5.0] * 3, [5.0] * 3


@pytest.mark.parametrize("name", ["BatchedPCABO", "BatchedVanillaBO"])
def test_batch_classes(name):
    from pcabo import batchrun
    cls = getattr(batchrun, name)
    r = cls([_Problem()], [1], 10, 4)
    assert (r._q, r._q_strategy) == (1, "kriging_believer")
    r = cls([_Problem()], [1], 10, 4, q=3, q_strategy="constant_liar_mean")
    assert (r._q, r._q_strategy) == (3, "constant_liar_mean")
    for kw in ({"q": 0}, {"q": 2.0}, {"q": "2"}, {"q": 2, "q_strategy": "believer"}):
        with pytest.raises(ValueError, match="q"):
            cls([_Problem()], [1], 10, 4, **kw)


def _main():
    spec = importlib.util.spec_from_file_location("pcabo_main_cli", os.path.join(ROOT, "para-ortho-pca-bo_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line(monkeypatch):
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "16"))     # (main.py sets a default: undone after)
    parse = _main().parse_arguments
    a = parse([])
    assert (a.q, a.q_strategy) == (1, "kriging_believer")
    a = parse(["--q", "3", "--q_strategy", "constant_liar_max"])
    assert (a.q, a.q_strategy) == (3, "constant_liar_max")
    for argv in (["--q", "0"], ["--q", "2", "--q_strategy", "thompson"], ["--q", "1.5"]):
        with pytest.raises(SystemExit):
            parse(argv)
