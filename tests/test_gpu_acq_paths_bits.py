"""Every acquisition path keeps the bits it had before the scalar maths of the acquisition (covariance, log-EI / PI / UCB chain)
moved into one header, acq_math.h: tests/golden/acq_paths_hashes.json was written by tools/gpu_acq_paths_hashes.py from the
library as it was, and is never regenerated for a change that is not meant to change arithmetic.  All three acquisitions, both
directions, Matern and RBF, the clamped variance and the three branches of log-EI, on acq_eval (q = 32, 40), gp_wait_eval
(q = 512, on two streams and on one), the same on a group-kernel context, Batch.gp_wait_eval and the device optimiser's lb_eval."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gpu_acq_paths_hashes", os.path.join(ROOT, "tools", "gpu_acq_paths_hashes.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "acq_paths_hashes.json")))["cases"]


@pytest.mark.parametrize("name", list(H.STATES))
def test_hashed_queries_reach_every_branch_of_the_chain(name):
    """No GPU.  On the tool's own float64 posterior, the 32 queries that every path evaluates fall into each branch of the scalar
    chain at the incumbent meant for it, with margins far beyond rounding: u > -1, -1e6 < u <= -1, u <= -1e6; PI's second incumbent
    leaves it between 1e-9 and 0.16 somewhere; state E, and only E, is under the variance floor at every query."""
    mu, sigma, clamped = H.chain_inputs(name)
    assert mu.shape == sigma.shape == clamped.shape == (32,)
    assert clamped.all() if name == "E" else not clamped.any()
    for maximize in (0, 1):
        inc = H.incumbents(name, maximize)
        u = {k: H.u_of(name, maximize, v) for k, v in inc.items()}
        assert np.count_nonzero(u["near"] > -0.5) >= 1
        assert np.count_nonzero((u["mid"] < -2.0) & (u["mid"] > -1e5)) == 32
        assert np.count_nonzero(u["far"] < -1e7) == 32
        assert np.count_nonzero((u["3sigma"] < -1.0) & (u["3sigma"] > -6.0)) >= 1
    cases = H.cases(name)                                    # (asserts the same while it builds the list)
    labels = [c[0] for c in cases]
    assert len(labels) == len(set(labels)) == 14
    assert set(labels) == set(GOLDEN[name])
    by = {c[0]: c for c in cases}
    for maximize in (0, 1):
        inc = H.incumbents(name, maximize)
        assert [by["log_ei,%d,%s" % (maximize, k)][3] for k in ("near", "mid", "far")] == [inc["near"], inc["mid"], inc["far"]]
        assert [by["pi,%d,%s" % (maximize, k)][3] for k in ("near", "3sigma")] == [inc["near"], inc["3sigma"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(H.STATES))
def test_every_acquisition_path_has_the_pinned_bits(native, name):
    got = H.compute_state(name)
    golden = GOLDEN[name]
    assert set(got) == set(golden)
    paths = 10 if H.STATES[name][1] <= 40 else 9          # no device optimiser beyond k = 40
    bad = [(case, path) for case in golden for path in golden[case] if got[case].get(path) != golden[case][path]]
    assert all(len(golden[case]) == paths and set(got[case]) == set(golden[case]) for case in golden)
    assert not bad, (name, len(bad), bad[:12])
