"""The posterior entry points keep the bits they had before their tile product (pcabo_internal.h: tile_product_f64, under the score
GEMM, k_post_cov and k_post_sample) and their host sequence (pcabo_api.hip: PostSite, post_enqueue, sample_enqueue) were written once
each: tests/golden/posterior_hashes.json was written by tools/gpu_posterior_hashes.py from the library as it was, and is never
regenerated for a change that is not meant to change arithmetic.  Mean, variance, covariance, samples and the ladder's rung, on a
context and on batches of three runs (one parked, one climbing the ladder alone; before and after the lock-step fit) and of one run."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gpu_posterior_hashes", os.path.join(ROOT, "tools", "gpu_posterior_hashes.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "posterior_hashes.json")))["cases"]


def _differences(got, golden):
    return [key for key in set(got) | set(golden) if got.get(key) != golden.get(key)]


def test_golden_holds_both_halves_of_the_ladder():
    """No GPU: the recorded cases reach the first rung and the climb, in a context and for the lone run of a batch."""
    rungs = [rec["rung"] for rec in GOLDEN.values() if "rung" in rec]
    assert 0.0 in rungs and any(r != 0.0 for r in rungs)
    for name in ("batch3_cond", "batch3_fit"):
        assert GOLDEN[name]["run0_noise0"]["rung"] == 0.0 and GOLDEN[name]["run2_noise0"]["rung"] != 0.0
    assert "covariance" not in GOLDEN["s4_plain_mean_var"]


@pytest.mark.gpu
def test_context_posterior_has_the_pinned_bits(native):
    got = H.context_cases(native)
    assert set(got) == {name for name in GOLDEN if not name.startswith("batch")}
    bad = {name: _differences(got[name], GOLDEN[name]) for name in got if got[name] != GOLDEN[name]}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("fitted", [False, True])
def test_batch_of_three_has_the_pinned_bits(native, fitted):
    got, golden = H.batch3_case(native, fitted), GOLDEN["batch3_fit" if fitted else "batch3_cond"]
    assert set(got) == set(golden) and got["k"] == golden["k"]
    bad = {run: _differences(got[run], golden[run]) for run in got if got[run] != golden[run]}
    assert not bad, bad


@pytest.mark.gpu
def test_batch_of_one_has_the_pinned_bits(native):
    got = H.batch1_case(native)
    assert got == GOLDEN["batch1"], _differences(got, GOLDEN["batch1"])
