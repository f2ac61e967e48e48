"""The lock-step GP hyperparameter fit of a batch (pcabo_batch_gp_mll / pcabo_batch_gp_fit, BatchedPCABO / BatchedVanillaBO
fit_gp=True, ExperimentRunner batched_fit_gp=True): what can be checked without a GPU - the ABI, the keywords, the flag."""
import importlib.util
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_fit_symbols_declared_and_exported(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    for name in ("pcabo_batch_gp_mll", "pcabo_batch_gp_fit"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in native.EXPORTS
        assert hasattr(native.LIB, name)
    assert hasattr(native.Batch, "gp_mll") and hasattr(native.Batch, "gp_fit")


def test_experiment_runner_takes_batched_fit_gp(native):
    from Algorithms import ExperimentRunner
    er = ExperimentRunner(algorithms=["pca"], dimensions=[10], problem_ids=[15], num_runs=30, progress=False,
                          batched=30, batched_fit_gp=True)
    assert er.batched_fit_gp is True and er.fit_gp is False
    er = ExperimentRunner(algorithms=["pca"], dimensions=[10], problem_ids=[15], num_runs=30, progress=False, batched=30)
    assert er.batched_fit_gp is False


@pytest.mark.parametrize("batched", [0, 1])
def test_batched_fit_gp_needs_batches(native, batched):
    from Algorithms import ExperimentRunner
    with pytest.raises(ValueError, match="batched"):
        ExperimentRunner(algorithms=["pca"], dimensions=[10], problem_ids=[15], num_runs=30, progress=False,
                         batched=batched, batched_fit_gp=True)


def test_fit_gp_with_batched_runs_is_still_refused(native):
    from Algorithms import ExperimentRunner
    with pytest.raises(ValueError, match="lock-step batches"):
        ExperimentRunner(algorithms=["pca"], dimensions=[10], problem_ids=[15], num_runs=30, progress=False,
                         batched=30, fit_gp=True)


def test_main_parses_batched_fit_gp(native):
    spec = importlib.util.spec_from_file_location("pcabo_main_cli_bf", os.path.join(ROOT, "para-ortho-pca-bo_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    saved = os.environ.get("GPU_MAX_HW_QUEUES")          # (main.py sets a default for the processes it drives)
    try:
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            os.environ.pop("GPU_MAX_HW_QUEUES", None)
        else:
            os.environ["GPU_MAX_HW_QUEUES"] = saved
    a = mod.parse_arguments(["--batched", "30", "--batched_fit_gp"])
    assert a.batched_fit_gp is True and a.fit_gp is False
    assert mod.parse_arguments([]).batched_fit_gp is False


def test_batch_drivers_take_fit_gp(native):
    from pcabo.batchrun import BatchedPCABO, BatchedVanillaBO, bench_block
    for cls in (BatchedPCABO, BatchedVanillaBO):
        assert inspect.signature(cls.__init__).parameters["fit_gp"].default is False
    assert inspect.signature(bench_block).parameters["fit_gp"].default is False
    from pcabo.bbob import BBOBProblem
    for kernel in ("group", "latency", "device", "device-twin"):
        r = BatchedPCABO([BBOBProblem(15, i, 10) for i in range(2)], [1, 2], 70, 30, acq_kernel=kernel, fit_gp=True)
        assert r.timing["fit"] == 0.0 and r.gp_hyperparameters == [None, None]
    assert BatchedPCABO([BBOBProblem(15, 0, 10)], [1], 70, 30).timing["fit"] == 0.0


@pytest.mark.parametrize("value", [4.966580630, 0.1, 1.0, -3.3333333333333335])
def test_constant_rows_pick_what_a_single_run_picks(native, value):
    """Raw samples of a nearly constant posterior (a fitted GP early in a run) all score the same value.  torch's reduction may
    round the mean of equal values and see std > 0 where the library's Welford pass sees exactly 0: the batch's pick must follow
    torch, as a single run does, and leave the run's generator where the single run's call leaves it."""
    import warnings
    import numpy as np
    from pcabo import initializers as I
    from pcabo.hostrng import HostMT
    vals = np.full((3, 512), value)
    vals[1] = np.linspace(0.0, 1.0, 512)                 # an ordinary row between two constant ones
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gens = [HostMT(100 + b) for b in range(3)]
        rows = I.initialize_q_batch_rows(vals, 10, gens)
        for b in range(3):
            g = HostMT(100 + b)
            one = I.initialize_q_batch(vals[b], 10, generator=g)
            assert np.array_equal(np.asarray(rows[b]), np.asarray(one)), b
            assert np.array_equal(np.asarray(g.get_state()), np.asarray(gens[b].get_state())), b
