"""Whole runs of PCA_BO and Vanilla_BO keep the bits they had before the part the two classes share was written once
(Algorithms/BayesianOptimization/DeviceBayesianOptimizer.py): tests/golden/single_run_hashes.json was written by tools/gpu_run_hashes.py
from the two classes as they were, and is never regenerated for a change that is not meant to change a run's arithmetic or the order
in which it consumes its generators.  Ten iterations of BBOB f15 per case: every keyword that selects another path, a run stepped
with _start / _bo_iteration / _finish that queries its model on the way (posterior, posterior_samples, loo, fantasy), and a PCA_BO run
that meets the out-of-bounds penalty."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gpu_run_hashes", os.path.join(ROOT, "tools", "gpu_run_hashes.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)
_FILE = json.load(open(os.path.join(ROOT, "tests", "golden", "single_run_hashes.json")))
GOLDEN, OOB_SEED = _FILE["cases"], _FILE["oob_seed"]
TRAJECTORY = {"x_evals", "f_evals", "lbfgsb_info", "n"}
VISIT = {"posterior", "posterior_samples", "loo", "fantasy_loo"}


def _differences(got, golden):
    return sorted(name for name in set(got) | set(golden) if got.get(name) != golden.get(name))


def test_golden_holds_every_case_of_both_classes():
    """No GPU: every keyword case and the visit case of both classes, each with what it has to pin; the out-of-bounds case at the
    seed the file names; PCA_BO's runs with k < d and a k that changes on the way."""
    oob = {"pca_oob_seed%d" % OOB_SEED} if OOB_SEED is not None else set()
    assert set(GOLDEN) == H.case_names("pca") | H.case_names("vanilla") | oob
    assert OOB_SEED is None or OOB_SEED in H.OOB_SEEDS
    iterations = H.BUDGET - H.N_DOE
    for name, rec in GOLDEN.items():
        cls, case = name.split("_", 1)
        extra = set(rec) - TRAJECTORY
        assert TRAJECTORY <= set(rec) and rec["n"] == H.BUDGET, name
        if cls == "pca":
            assert len(rec["k"]) == iterations and all(1 <= k < H.DIM["pca"] for k in rec["k"]), name
            extra -= {"k"}
        want = {"gp_hyperparameters"} if case.startswith("fit") else {"trace_n", "trace_best_f"} if case == "trace" else \
            VISIT if case == "visit" else set()
        assert extra == want, name
        if case == "trace":
            assert rec["trace_n"] == list(range(H.N_DOE, H.BUDGET)), name
        if case == "visit":
            assert all(isinstance(rec[q], dict) and rec[q] for q in VISIT), name
            assert {"mean", "variance", "covariance"} <= set(rec["posterior"]) and "samples" in rec["posterior_samples"], name
    assert len(set(GOLDEN["pca_default"]["k"])) > 1 and GOLDEN["pca_components3"]["k"] == [3] * iterations
    # the keywords change the path, not (always) the run: these are the same trajectory by other routes
    for same in ("not_resident", "unfused", "late_scoring", "no_engine_guess", "no_prefetch"):
        assert GOLDEN["pca_" + same]["x_evals"] == GOLDEN["pca_default"]["x_evals"], same
    for cls in ("pca", "vanilla"):
        assert {key: GOLDEN[cls + "_visit"][key] for key in TRAJECTORY} == {key: GOLDEN[cls + "_default"][key] for key in TRAJECTORY}
        assert len({GOLDEN["%s_%s" % (cls, c)]["x_evals"] for c in ("default", "fit", "fit_ard", "pi", "ucb")}) == 5, cls


@pytest.mark.gpu
@pytest.mark.parametrize("cls", ["pca", "vanilla"])
def test_single_runs_have_the_pinned_bits(native, cls):
    got = H.class_cases(cls, OOB_SEED if cls == "pca" else None)
    golden = {name: rec for name, rec in GOLDEN.items() if name.startswith(cls + "_")}
    assert set(got) == set(golden)
    bad = {name: _differences(got[name], golden[name]) for name in got if got[name] != golden[name]}
    assert not bad, bad
