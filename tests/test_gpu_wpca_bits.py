"""The weighted PCA keeps its bits: tests/golden/wpca_bits_hashes.json was written by tools/gpu_wpca_hashes.py from the library
as it was before the round of `k_jacobi` was rewritten (lanes per pair, number of waves, LDS flag, prologue and epilogue), and is
never regenerated for a change that is not meant to change arithmetic.  Hashed: data_mean, pca_mean, components, evr, k and Z of
`Context.wpca`, a cold call and two warm calls with one row appended each, at

- d in {1, 2, 3, 5, 16, 17, 32, 33, 40, 48, 49, 63, 64, 65, 100, 127, 128}: odd d (the virtual column), every rows-per-lane
  boundary of 16 (and of 8) lanes per pair, the d = 64 / 65 split, the staged (d <= 64) and the unstaged warm start;
- n in {2, d - 1, d, d + 1, 3 d} (<= 400): rcount = n < d and beyond;
- all four generators (`twin`: tied eigenvalues, the tie order of the selection);
- after a rank-deficient call and after collapsed start vectors, data times 2^270 (range guard), `n_components` fixed;
- a batch of three different runs (`wpca_gp_condition_begin` -> `wpca_results`), which must equal the three single calls.

A case id missing from the golden file is a failure; nothing here skips."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gpu_wpca_hashes", os.path.join(ROOT, "tools", "gpu_wpca_hashes.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "wpca_bits_hashes.json")))["cases"]

@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=H.MAX_N, max_d=H.MAX_D, max_q=64)
    yield c
    c.close()


def _compare(got):
    missing = [cid for cid in got if cid not in GOLDEN]
    assert not missing, ("case ids without a golden entry", missing[:12])
    bad = [(cid, [i for i, (a, b) in enumerate(zip(got[cid], GOLDEN[cid])) if a != b] or "length")
           for cid in got if got[cid] != GOLDEN[cid]]
    assert not bad, (len(bad), bad[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("d", H.GRID_D)
def test_grid_cold_then_two_warm_calls_have_the_pinned_bits(ctx, d):
    got = H.compute_d(ctx, d)
    assert len(got) == 4 * len(H.grid_n(d)) and all(len(v) == 3 for v in got.values())
    _compare(got)


@pytest.mark.gpu
@pytest.mark.parametrize("what", H.EXTRAS)
def test_special_calls_have_the_pinned_bits(ctx, what):
    got = H.compute_extra(ctx, what)
    assert got
    _compare(got)


@pytest.mark.gpu
def test_batch_of_three_runs_equals_three_single_calls(native):
    got = H.compute_batch(native)
    assert len(got["batch"]) == 6
    assert got["batch"] == got["single"], [i for i in range(6) if got["batch"][i] != got["single"][i]]
    _compare(got)


def test_golden_file_covers_exactly_the_cases_of_the_tool():
    """No GPU."""
    ids = {"%s-d%d-n%d" % (g, d, n) for g in H.R.GENERATORS for d in H.GRID_D for n in H.grid_n(d)}
    extra = set(GOLDEN) - ids
    assert ids <= set(GOLDEN), sorted(ids - set(GOLDEN))[:12]
    assert {"batch", "single"} <= extra and len(extra) == 10, sorted(extra)
