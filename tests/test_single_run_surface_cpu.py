"""What PCA_BO and Vanilla_BO accept, refuse and resolve without a device: the part of the two classes that lives once in
Algorithms/BayesianOptimization/DeviceBayesianOptimizer.py, with the run guard (pcabo/gcguard.py) and the acquisition-name resolver
(pcabo/acqopt.py) they share with the lock-step batches.  The exception types are those the two classes raised while each had its
own copy of this code."""
import gc

import pytest
import torch

from Algorithms import PCA_BO, Vanilla_BO
from Algorithms.BayesianOptimization import PCA_BO as pca_module
from Algorithms.BayesianOptimization.DeviceBayesianOptimizer import (AnalyticAcquisitionFunction, DeviceBayesianOptimizer,
                                                                     LogExpectedImprovement, ProbabilityOfImprovement,
                                                                     UpperConfidenceBound)
from pcabo.acqopt import acquisition_long_name
from pcabo.gcguard import RunGuard

both = pytest.mark.parametrize("cls", [PCA_BO, Vanilla_BO])
CLASSES = {"EI": LogExpectedImprovement, "PI": ProbabilityOfImprovement, "UCB": UpperConfidenceBound,
           "expected_improvement": LogExpectedImprovement, "probability_of_improvement": ProbabilityOfImprovement,
           "upper_confidence_bound": UpperConfidenceBound}


@both
def test_torch_config_follows_smoke_test(cls, monkeypatch):
    monkeypatch.delenv("SMOKE_TEST", raising=False)
    cfg = cls(budget=10).torch_config
    assert (cfg["NUM_RESTARTS"], cfg["RAW_SAMPLES"], cfg["BATCH_SIZE"]) == (10, 512, 3) and cfg["SMOKE_TEST"] is None
    monkeypatch.setenv("SMOKE_TEST", "1")
    cfg = cls(budget=10).torch_config
    assert (cfg["NUM_RESTARTS"], cfg["RAW_SAMPLES"], cfg["BATCH_SIZE"]) == (2, 32, 2) and cfg["SMOKE_TEST"] == "1"


@both
@pytest.mark.parametrize("kwargs", [{"fantasy_points": -1}, {"ard": True}, {"ucb_beta": 1.0},
                                    {"acquisition_function": "UCB", "ucb_beta": -1.0},
                                    {"acquisition_function": "UCB", "ucb_beta": float("nan")},
                                    {"acquisition_function": "thompson"}, {"acquisition_function": "ei"}])
def test_constructor_refusals(cls, kwargs):
    with pytest.raises(ValueError):
        cls(budget=10, **kwargs)


@both
def test_odd_name_keeps_the_wording_of_its_class(cls):
    with pytest.raises(ValueError) as e:
        cls(budget=10, acquisition_function=" thompson ")
    assert str(e.value) == ("Oddly defined name" if cls is PCA_BO else "Oddly defined name thompson")


@both
def test_accepted_keywords(cls):
    """ucb_beta = 0 is a value (a pure mean); unknown keywords travel on to AbstractAlgorithm, which ignores them."""
    assert cls(budget=10, acquisition_function="UCB", ucb_beta=0.0).acquisition_function_class is UpperConfidenceBound
    opt = cls(budget=10, n_DoE=4, device=0, record_trace=True, torch_threads=None, gc_freeze=False, resident=False, fantasy_points=2,
              fit_gp=True, ard=True, verbose=False, some_other_keyword=3)
    assert opt.budget == 10 and opt.n_DoE == 4 and opt.device_context is None and opt.gp_hyperparameters is None
    assert opt.trace == [] and opt.lbfgsb_info == []
    assert opt.phase_breakdown == ({"sobol": 0.0, "raw_eval": 0.0, "init_pick": 0.0, "lbfgsb": 0.0} if cls is PCA_BO else {})
    assert list(opt.timing_logs) == cls.TIME_PROFILES
    assert isinstance(opt, DeviceBayesianOptimizer)


@both
@pytest.mark.parametrize("name", sorted(CLASSES))
def test_names_resolve_to_their_classes(cls, name):
    opt = cls(budget=10, acquisition_function=" %s " % name)
    assert opt.acquisition_function_class is CLASSES[name]
    assert opt.acquisition_function_name == acquisition_long_name(name) and opt.acquisition_function_name in CLASSES
    opt.acquisition_function_name = "PI"
    assert opt.acquisition_function_class is ProbabilityOfImprovement


def test_pca_bo_still_exports_what_moved():
    for name in ("ALLOWED_ACQUISITION_FUNCTION_STRINGS", "ALLOWED_SHORTHAND_ACQUISITION_FUNCTION_STRINGS", "AnalyticAcquisitionFunction",
                 "LogExpectedImprovement", "ProbabilityOfImprovement", "UpperConfidenceBound", "LENGTHSCALE", "NOISE", "OOB_PENALTY",
                 "checked_ard", "fit_gp_hyperparameters"):
        assert hasattr(pca_module, name), name
    assert pca_module.UpperConfidenceBound is UpperConfidenceBound


@both
def test_acquisition_function_must_be_a_descriptor(cls):
    opt = cls(budget=10)
    with pytest.raises(AttributeError, match="does not inherit from 'AnalyticAcquisitionFunction'"):
        opt.acquisition_function = object()
    acq = LogExpectedImprovement(best_f=1.0)
    opt.acquisition_function = acq
    assert opt.acquisition_function is acq and isinstance(acq, AnalyticAcquisitionFunction)


@both
@pytest.mark.parametrize("query", ["posterior", "posterior_samples", "loo", "fantasy"])
def test_model_queries_need_an_open_run(cls, query):
    opt = cls(budget=10)                   # (no run yet: no dimension either - the refusal comes before X is looked at)
    with pytest.raises(RuntimeError, match="^%s: no run is open, or the model of the current iteration is not conditioned yet$" % query):
        if query == "loo":
            opt.loo()
        elif query == "fantasy":
            with opt.fantasy([[0.0, 0.0]]):
                pass
        else:
            getattr(opt, query)([[0.0, 0.0]])


def test_acq_kernel_is_checked():
    with pytest.raises(ValueError, match="acq_kernel"):
        PCA_BO(budget=10, acq_kernel="x")
    assert PCA_BO(budget=10, acq_kernel="group").device_context is None


def test_run_guard_puts_everything_back():
    threads, thresholds = torch.get_num_threads(), gc.get_threshold()
    try:
        torch.set_num_threads(6)
        RunGuard(4, True).leave()                            # leave without enter: nothing to undo
        assert (torch.get_num_threads(), gc.get_threshold(), gc.get_freeze_count()) == (6, thresholds, 0)
        guard = RunGuard(4, True)
        for _ in range(2):                                   # (entered twice, as after a start that is repeated)
            guard.enter()
        assert torch.get_num_threads() == 4 and gc.get_threshold()[0] >= thresholds[0] and gc.get_freeze_count() > 0
        for _ in range(2):
            guard.leave()
            assert (torch.get_num_threads(), gc.get_threshold(), gc.get_freeze_count()) == (6, thresholds, 0)
        guard = RunGuard(8, False)                           # nothing to lower, collector left alone
        guard.enter()
        assert (torch.get_num_threads(), gc.get_threshold(), gc.get_freeze_count()) == (6, thresholds, 0)
        guard.leave()
        guard = RunGuard(None, False)
        guard.enter()
        guard.leave()
        assert (torch.get_num_threads(), gc.get_threshold()) == (6, thresholds)
    finally:
        torch.set_num_threads(threads)


class _Problem:
    class meta_data:
        n_variables = 3


@pytest.mark.parametrize("name", ["thompson", "ei", ""])
def test_batch_refuses_an_odd_name_through_the_shared_resolver(name):
    from pcabo.batchrun import BatchedPCABO, BatchedVanillaBO
    with pytest.raises(ValueError, match="^Oddly defined name$"):
        acquisition_long_name(name)
    for cls in (BatchedPCABO, BatchedVanillaBO):
        with pytest.raises(ValueError, match="^Oddly defined name$"):
            cls([_Problem()], [1], 10, 4, acquisition_function=name)
    with pytest.raises(ValueError, match="^Oddly defined name$"):          # (UCB without ucb_beta: refused where the batch is built)
        BatchedPCABO([_Problem()], [1], 10, 4, acquisition_function="UCB")
