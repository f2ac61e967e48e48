"""The upper-confidence-bound acquisition (`ucb_beta=`), what can be checked without a GPU: the ABI constant, the keyword
through every layer, and the host optimiser on UCB surfaces against scipy."""
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

import pcabo_oracle as O
from pcabo.bbob import BBOBProblem
from ucb_reference import CPU_STATES, bbob_state, kappa_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. header and binding ------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_ucb(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    assert re.search(r"\bPCABO_ACQ_UCB\s*=\s*2\b", header)
    assert (native.ACQ_LOG_EI, native.ACQ_PI, native.ACQ_UCB) == (0, 1, 2)
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2          # additive: the version stays


# ---- 2. plumbing without a device -----------------------------------------------------------------------------------------
def test_optimisers_construct_with_ucb_beta_and_expose_kappa(native):
    from Algorithms import PCA_BO, Vanilla_BO
    from Algorithms.BayesianOptimization.PCA_BO import LogExpectedImprovement, UpperConfidenceBound
    from pcabo.batchrun import BatchedPCABO, BatchedVanillaBO
    kappa = float(torch.as_tensor(2.0).sqrt())
    assert kappa == kappa_of(2.0) and kappa != 2.0 ** 0.5                     # the float32 root, not the float64 one
    for name in ("UCB", "upper_confidence_bound"):
        for cls in (PCA_BO, Vanilla_BO):
            opt = cls(budget=20, n_DoE=8, acquisition_function=name, ucb_beta=2.0)
            assert opt.acquisition_function_name == "upper_confidence_bound"
            assert opt.acquisition_function_class is UpperConfidenceBound
        for cls in (BatchedPCABO, BatchedVanillaBO):
            r = cls([BBOBProblem(15, i, 6) for i in range(2)], [1, 2], 20, 10, acquisition_function=name, ucb_beta=2.0)
            assert r.acq_code == native.ACQ_UCB and r._acq_scalars() == [kappa, kappa]
    acq = UpperConfidenceBound(model=None, beta=2.0, maximize=False)           # botorch's own signature
    assert acq.acq_code == native.ACQ_UCB and acq.device_scalar == kappa and acq.maximize is False
    assert UpperConfidenceBound(beta=0.0).device_scalar == 0.0
    ei = LogExpectedImprovement(model=None, best_f=3.5, maximize=False)
    assert ei.device_scalar == 3.5                                             # EI / PI: the scalar is best_f, as before
    with pytest.raises(TypeError):                                             # the reference's call: still a TypeError
        UpperConfidenceBound(model=None, best_f=1.0, maximize=False)


@pytest.mark.parametrize("beta", [-1.0, float("nan"), float("inf")])
def test_bad_ucb_beta_is_a_value_error(native, beta):
    from Algorithms import ExperimentRunner, PCA_BO, Vanilla_BO
    from pcabo.batchrun import BatchedPCABO
    for cls in (PCA_BO, Vanilla_BO):
        with pytest.raises(ValueError):
            cls(budget=20, n_DoE=8, acquisition_function="UCB", ucb_beta=beta)
    with pytest.raises(ValueError):
        BatchedPCABO([BBOBProblem(15, 0, 6)], [1], 20, 10, acquisition_function="UCB", ucb_beta=beta)
    with pytest.raises(ValueError):
        ExperimentRunner(algorithms=["pca"], dimensions=[5], problem_ids=[15], num_runs=1, progress=False,
                         acquisition_function="upper_confidence_bound", ucb_beta=beta)


@pytest.mark.parametrize("name", ["EI", "expected_improvement", "PI"])
def test_ucb_beta_with_another_acquisition_is_a_value_error(native, name):
    from Algorithms import ExperimentRunner, PCA_BO, Vanilla_BO
    from pcabo.batchrun import BatchedPCABO
    for cls in (PCA_BO, Vanilla_BO):
        with pytest.raises(ValueError):
            cls(budget=20, n_DoE=8, acquisition_function=name, ucb_beta=2.0)
    with pytest.raises(ValueError):
        BatchedPCABO([BBOBProblem(15, 0, 6)], [1], 20, 10, acquisition_function=name, ucb_beta=2.0)
    with pytest.raises(ValueError):
        ExperimentRunner(algorithms=["pca"], dimensions=[5], problem_ids=[15], num_runs=1, progress=False,
                         acquisition_function=name, ucb_beta=2.0)


def test_batch_drivers_without_ucb_beta_keep_their_value_error(native):
    from pcabo.batchrun import BatchedPCABO, BatchedVanillaBO
    for cls in (BatchedPCABO, BatchedVanillaBO):
        for name in ("UCB", "upper_confidence_bound"):
            with pytest.raises(ValueError, match="Oddly defined name"):
                cls([BBOBProblem(15, 0, 6)], [1], 20, 10, acquisition_function=name)


def test_experiment_runner_hands_ucb_beta_on_and_records_it_only_when_set(native, tmp_path, monkeypatch):
    """The optimisers are replaced by a stand-in that evaluates one point (no device): what reaches them, and what the
    experiment's JSON files hold with and without the keyword."""
    er_mod = importlib.import_module("Algorithms.Experiment.ExperimentRunner")
    seen = []

    class StandIn:
        TIME_PROFILES = ["SingleTaskGP", "optimize_acqf"]

        def __init__(self, **kw):
            seen.append(kw)
            self.total_times = {p: 0.0 for p in self.TIME_PROFILES}
            self.current_best = 0.0

        def __call__(self, problem):
            self.current_best = problem(np.zeros(problem.meta_data.n_variables))

    monkeypatch.setattr(er_mod, "PCA_BO", StandIn)
    monkeypatch.setattr(er_mod, "Vanilla_BO", StandIn)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    metas = {}
    for tag, extra in (("with", {"ucb_beta": 2.0}), ("without", {})):
        seen.clear()
        er = er_mod.ExperimentRunner(algorithms=["pca", "vanilla"], dimensions=[5], problem_ids=[15], num_runs=2, progress=False,
                                     root_dir=str(tmp_path / tag), acquisition_function="upper_confidence_bound", **extra)
        assert er.ucb_beta == extra.get("ucb_beta")
        er.run_experiment()
        assert len(seen) == 4
        assert all(kw.get("ucb_beta") == 2.0 for kw in seen) if extra else all("ucb_beta" not in kw for kw in seen)
        for alg in ("pca", "vanilla"):
            path = os.path.join(str(tmp_path / tag), f"{alg}-experiment", "IOHprofiler_f15_RastriginRotated.json")
            metas[tag, alg] = (open(path).read(), json.load(open(path)))
    for alg in ("pca", "vanilla"):
        text, meta = metas["with", alg]
        assert {"ucb_beta": "2.0"} in meta["experiment_attributes"] and "ucb_beta" in meta["run_attributes"]
        assert all(run["ucb_beta"] == 2.0 for run in meta["scenarios"][0]["runs"])
        text, meta = metas["without", alg]
        assert "ucb_beta" not in text


def test_command_line_takes_ucb_beta():
    import main
    a = main.parse_arguments(["--ucb_beta", "2"])
    assert a.ucb_beta == 2.0 and isinstance(a.ucb_beta, float)
    assert main.parse_arguments([]).ucb_beta is None
    a = main.parse_arguments(["--acquisition", "upper_confidence_bound", "--ucb_beta", "0.25", "--batched", "2"])
    assert (a.acquisition, a.ucb_beta, a.batched) == ("upper_confidence_bound", 0.25, 2)


# ---- 3. the host optimiser on UCB surfaces --------------------------------------------------------------------------------
@pytest.mark.parametrize("fid,d,n,beta,maximize", CPU_STATES)
def test_host_lbfgsb_on_ucb_surfaces_takes_scipys_path(native, fid, d, n, beta, maximize):
    """10 initial conditions from 64 raw samples, two joint groups of 5: csrc/lbfgsb.cpp over the reference UCB against
    botorch's gen_candidates_scipy (scipy's L-BFGS-B) over the same surface.  Measured on the library before this acquisition
    existed: iteration and evaluation counts identical in 12 of 12 groups, end points within 1.6e-7 relative (most <= 1e-11);
    asserted: identical counts, end points within the project's candidate tolerance 1e-5."""
    torch.set_num_threads(1)
    acq, bounds = bbob_state(fid, d, n, beta, maximize)
    k = bounds.shape[1]
    torch.manual_seed(3)
    ics = O.gen_batch_initial_conditions(acq, bounds, 10, 64, 5)
    assert ics.shape == (10, k)
    for s in (0, 5):
        cand, vals, failed, tr = O.gen_candidates_scipy(ics[s:s + 5], acq, bounds)
        assert not failed
        lo, hi = np.tile(bounds[0], 5), np.tile(bounds[1], 5)

        def fun(x):
            v, g = acq.value_and_grad(x.reshape(5, k))
            return -float(v.sum()), -g.reshape(-1)

        mine = native.lbfgsb_minimize(fun, np.clip(ics[s:s + 5].reshape(-1), lo, hi), list(zip(lo, hi)), maxiter=200)
        x = np.clip(mine["x"].reshape(5, k), bounds[0], bounds[1])
        err = float(np.abs(x - cand).max() / max(1.0, np.abs(cand).max()))
        print("[UCB f%d d=%d n=%d beta=%g %s, group %d] scipy nit/nfev %d/%d, host %d/%d, end points %.2e"
              % (fid, d, n, beta, "max" if maximize else "min", s // 5, tr.nit, tr.nfev, mine["nit"], mine["nfev"], err))
        assert (mine["nit"], mine["nfev"]) == (tr.nit, tr.nfev)
        assert err <= 1e-5
