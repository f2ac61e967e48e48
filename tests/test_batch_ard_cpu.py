"""The lock-step ARD fit of a batch (pcabo_batch_gp_mll_ard / pcabo_batch_gp_fit_ard, Batch.gp_mll_ard / Batch.gp_fit_ard,
BatchedPCABO / BatchedVanillaBO fit_gp=True, batched_ard=True, ExperimentRunner batched_fit_gp=True, batched_ard=True): what can
be checked without a GPU - the ABI, the keywords, the flag, and the batch driver over the scripted batch of tests/lockstep_fake.py."""
import importlib.util
import inspect
import os
import re
import warnings

import numpy as np
import pytest

import lockstep_fake as LF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNNER = dict(algorithms=["pca"], dimensions=[10], problem_ids=[15], num_runs=30, progress=False)


def test_batch_ard_symbols_declared_and_exported(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    for name in ("pcabo_batch_gp_mll_ard", "pcabo_batch_gp_fit_ard"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header)
        assert m and re.search(r"\bint\s+ld_theta\b", m.group(1)), name
        assert name in native.EXPORTS
        assert hasattr(native.LIB, name)
    assert hasattr(native.Batch, "gp_mll_ard") and hasattr(native.Batch, "gp_fit_ard")
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2


def test_batched_ard_needs_the_fit(native):
    from Algorithms import ExperimentRunner
    from pcabo.batchrun import BatchedPCABO, BatchedVanillaBO
    for cls in (BatchedPCABO, BatchedVanillaBO):
        assert inspect.signature(cls.__init__).parameters["batched_ard"].default is False
        with pytest.raises(ValueError, match="fit_gp"):
            cls([], [], budget=20, n_DoE=10, batched_ard=True)
    with pytest.raises(ValueError, match="batched_fit_gp"):
        ExperimentRunner(batched=30, batched_ard=True, **RUNNER)
    with pytest.raises(ValueError, match="batched"):                     # (no batches: batched_fit_gp itself is refused)
        ExperimentRunner(batched=0, batched_fit_gp=True, batched_ard=True, **RUNNER)
    with pytest.raises(ValueError, match="batched_fit_gp"):                # the single runs' fit does not switch it on
        ExperimentRunner(batched=0, fit_gp=True, batched_ard=True, **RUNNER)
    er = ExperimentRunner(batched=30, batched_fit_gp=True, batched_ard=True, **RUNNER)
    assert er.batched_ard is True and er.ard is False and er.batched_fit_gp is True
    assert ExperimentRunner(batched=30, batched_fit_gp=True, **RUNNER).batched_ard is False


def test_ard_on_the_batched_classes_and_runner_still_raises(native):
    from Algorithms import ExperimentRunner
    from pcabo.batchrun import BatchedPCABO, BatchedVanillaBO
    for cls in (BatchedPCABO, BatchedVanillaBO):
        with pytest.raises(ValueError, match="PCA_BO / Vanilla_BO"):
            cls([], [], budget=20, n_DoE=10, fit_gp=True, ard=True)
        with pytest.raises(ValueError, match="PCA_BO / Vanilla_BO"):
            cls([], [], budget=20, n_DoE=10, fit_gp=True, ard=True, batched_ard=True)
    with pytest.raises(ValueError, match="PCA_BO / Vanilla_BO"):
        ExperimentRunner(batched=30, batched_fit_gp=True, ard=True, **RUNNER)
    with pytest.raises(ValueError, match="PCA_BO / Vanilla_BO"):
        ExperimentRunner(batched=30, batched_fit_gp=True, batched_ard=True, ard=True, **RUNNER)


def test_main_parses_batched_ard(native):
    spec = importlib.util.spec_from_file_location("pcabo_main_cli_bard", os.path.join(ROOT, "para-ortho-pca-bo_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    saved = os.environ.get("GPU_MAX_HW_QUEUES")          # (main.py sets a default for the processes it drives)
    try:
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            os.environ.pop("GPU_MAX_HW_QUEUES", None)
        else:
            os.environ["GPU_MAX_HW_QUEUES"] = saved
    a = mod.parse_arguments(["--batched", "30", "--batched_fit_gp", "--batched_ard"])
    assert a.batched_ard is True and a.batched_fit_gp is True and a.ard is False
    assert mod.parse_arguments(["--batched", "30", "--batched_fit_gp"]).batched_ard is False
    for argv in (["--batched_ard"], ["--batched", "30", "--batched_ard"], ["--batched_fit_gp", "--batched_ard"],
                 ["--batched", "1", "--batched_fit_gp", "--batched_ard"], ["--fit_gp", "--ard", "--batched_ard"]):
        with pytest.raises(SystemExit):
            mod.parse_arguments(argv)


class ArdFakeBatch(LF.FakeBatch):
    """The scripted batch with the ARD fit: Batch.gp_fit_ard's dicts (one lengthscale per reduced input of the run)."""
    ard_calls = []

    def gp_fit(self, theta0=None):
        raise AssertionError("a batch with batched_ard=True fits through gp_fit_ard")

    def gp_fit_ard(self, theta0=None):
        self._log("gp_fit_ard", theta0)
        type(self).ard_calls.append((self.n, [int(k) for k in self.k]))
        self.fit_rounds = 40 + self.n % 3
        out = []
        for b in range(self.B):
            if not self.active[b]:
                out.append({"status": -1})
                continue
            status = self._event("fit_status", b)
            if status:
                out.append({"status": int(status)})
                continue
            flag = self._event("fit_warnflag", b) or 0
            k = int(self.k[b])
            theta = np.r_[0.01 + 1e-3 * b, 0.1, 0.5 * np.arange(k) - 0.25 * self.n]
            out.append({"theta": theta, "noise": float(theta[0]), "mean_constant": float(theta[1]),
                        "lengthscales": np.log1p(np.exp(theta[2:])), "loss": 1.0 + b, "iterations": 30 + b,
                        "evaluations": 60 + (self.n + b) % 9, "warnflag": int(flag), "task": 3 if flag else 1, "status": 0})
        return out


@pytest.mark.parametrize("cls", ["pca", "vanilla"])
def test_batch_driver_fits_ard_once_per_iteration_and_keeps_the_lengthscales(native, monkeypatch, cls):
    from pcabo import batchrun
    from pcabo.bbob import BBOBProblem
    monkeypatch.setattr(native, "Batch", ArdFakeBatch)
    ArdFakeBatch.script, ArdFakeBatch.created, ArdFakeBatch.ard_calls = dict(LF.FIT_SCRIPT), [], []
    Driver = batchrun.BatchedPCABO if cls == "pca" else batchrun.BatchedVanillaBO
    r = Driver([BBOBProblem(LF.FID, i, LF.DIM) for i in range(LF.B)], [1000 * LF.FID + 10 * LF.DIM + i for i in range(LF.B)],
               LF.BUDGET, LF.N_DOE, acq_kernel="group", fit_gp=True, batched_ard=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        r.run()
    (bt,) = ArdFakeBatch.created
    iterations = LF.BUDGET - LF.N_DOE
    assert [n for n, _ in ArdFakeBatch.ard_calls] == list(range(LF.N_DOE, LF.BUDGET))          # once per iteration, no gp_fit
    assert sum(line.startswith("gp_fit_ard") for line in bt.log) == iterations
    assert sorted(e for e in bt.fired if e[0].startswith("fit_")) == sorted(LF.FIT_SCRIPT)
    assert r.failed[1] is not None and "fit failed" in r.failed[1][1]                          # ("fit_status", 1, 19): parked
    flagged = [str(w.message) for w in caught if "did not converge" in str(w.message)]
    assert len(flagged) == 2                                                                   # the two warnflags: iterate kept
    last_n, last_k = ArdFakeBatch.ard_calls[-1]
    for b in (0, 2, 3):
        hp = r.gp_hyperparameters[b]
        assert hp["lengthscales"].shape == (last_k[b],) and "lengthscale" not in hp, b
        assert hp["theta"].shape == (2 + last_k[b],) and hp["theta"][2] == -0.25 * last_n
    assert r.gp_hyperparameters[1]["theta"][2] == -0.25 * 18                                   # its last fit before it was parked
    assert r.fit_rounds == sum(40 + n % 3 for n in range(LF.N_DOE, LF.BUDGET)) and r.timing["fit"] > 0.0
