"""The GP fit keeps the bits it had before it was written once for shared and per-input lengthscales (kernels_fit.hip: one
k_mll_grad / k_mll_finish pair; host_side.h: one mll_theta_ok, mll_assemble and FitRun; pcabo_api.hip: one launch, evaluation and
fit body): tests/golden/fit_hashes.json was written by tools/gpu_fit_hashes.py from the library as it was, and is never regenerated
for a change that is not meant to change arithmetic.  Loss, gradient, theta and the info quadruple of both forms' evaluations and
fits on a context, and of the lock-step evaluation and fit of a batch of three runs (different k, one parked)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gpu_fit_hashes", os.path.join(ROOT, "tools", "gpu_fit_hashes.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fit_hashes.json")))["cases"]


def _differences(got, golden):
    return sorted(name for name in set(got) | set(golden) if got.get(name) != golden.get(name))


def test_golden_holds_both_forms_the_linear_branch_and_the_batch():
    """No GPU: every shape at every theta in both forms, rho = 25 among them; every fit state from every start in both forms, the
    start outside the domain refused; the batch's evaluations, fits and rounds with run 1 parked."""
    evals = {name: rec for name, rec in GOLDEN.items() if name.startswith("eval_")}
    assert set(evals) == {"eval_n%d_k%d_t%d" % (n, k, i) for n, k in H.SHAPES for i in range(len(H.RHOS))}
    for name, rec in evals.items():
        assert set(rec["scalar"]) == set(rec["ard"]) == {"loss", "grad", "theta"}, name
        assert (rec["rho"] == 25.0) == (rec["rho_max"] == 25.0) == name.endswith("_t4"), name
    fits = {name: rec for name, rec in GOLDEN.items() if name.startswith("fit_")}
    assert set(fits) == {"fit_n%d_k%d_%s" % (n, k, start) for _, n, k in H.FIT_STATES for start in ("default", "seeded", "out")}
    for name, rec in fits.items():
        for form in ("scalar", "ard"):
            if name.endswith("_out"):
                assert rec[form] == {"status": -1}, name
            else:
                assert len(rec[form]["info"]) == 4 and rec[form]["info"][1] > 1, name
    batch = GOLDEN["batch3"]
    assert len(set(batch["k"])) >= 2 and batch["fit_rounds"] >= max(batch["fit_run%d" % b]["info"][1] for b in (0, 2))
    assert set(batch) == {"k", "fit_rounds"} | {"%s_run%d" % (what, b) for what in ("mll0", "mll2", "fit") for b in (0, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("cases", ["eval_cases", "fit_cases"])
def test_context_fit_has_the_pinned_bits(native, cases):
    got = getattr(H, cases)(native)
    golden = {name: rec for name, rec in GOLDEN.items() if name.startswith(cases[:-5])}
    assert set(got) == set(golden)
    bad = {name: _differences(got[name], golden[name]) for name in got if got[name] != golden[name]}
    assert not bad, bad


@pytest.mark.gpu
def test_batch_of_three_has_the_pinned_bits(native):
    got = H.batch3_case(native)
    assert got == GOLDEN["batch3"], _differences(got, GOLDEN["batch3"])
