"""GP posterior queries (pcabo_gp_posterior / pcabo_batch_gp_posterior), host side: the reference of tests/posterior_reference.py is
consistent with the oracle and with itself, and the surface exists from the header to the optimiser classes.  The device results are
checked against this reference in tests/test_gpu_posterior.py."""
import os
import re

import numpy as np
import pytest
import torch

import pcabo_oracle as O
from ard_reference import ard_state
from posterior_reference import conditioned_on_one_more, posterior
from ucb_reference import bbob_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    """(GP, Z, q x k queries): a wPCA state with data-derived bounds (Matern), a seeded state with user bounds (RBF)."""
    ref, box = bbob_state(15, 6, 30, 2.0, False)
    gp = ref.gp
    Xa = np.random.default_rng(5).uniform(box[0], box[1], size=(40, gp.k))
    Z, y = ard_state(2, 65, 5)
    nb = np.vstack([np.full(5, -2.5), np.full(5, 3.0)])
    gb = O.ExactGP(Z, y, nb, kernel="rbf")
    Xb = np.random.default_rng(6).uniform(-2.0, 2.0, size=(33, 5))
    Xb[1] = Xb[0] + 1e-7                                   # two queries that almost coincide
    return [(gp, (gp.Zn * gp.coef + gp.lo).numpy(), Xa), (gb, Z, Xb)]


@pytest.fixture(scope="module")
def cases():
    torch.set_num_threads(4)
    return _cases()


def test_reference_agrees_with_the_oracle_and_with_itself(cases):
    for gp, _, X in cases:
        for noise in (False, True):
            r = posterior(gp, X, noise)
            sy2 = r["y_std"] ** 2
            cov = r["covariance"]
            assert np.array_equal(np.diag(cov), r["raw_variance"])
            assert np.array_equal(r["variance"], np.maximum(r["raw_variance"], 1e-10))
            assert np.abs(cov - cov.T).max() <= 1e-14 * sy2
            assert np.linalg.eigvalsh(0.5 * (cov + cov.T)).min() >= -1e-12 * sy2
            om, ov = gp.posterior(torch.from_numpy(X))
            assert np.abs(r["mean"] - om.numpy()).max() <= 1e-13 * max(1.0, np.abs(om.numpy()).max())
            if noise:
                assert np.abs((r["raw_variance"] - posterior(gp, X)["raw_variance"]) / sy2 - gp.noise).max() <= 1e-14
            else:
                assert np.abs(r["variance"] - ov.numpy()).max() <= 1e-13 * sy2


def test_fantasy_identity(cases):
    """Conditioning on an observation at x lowers the variance at x' by cov(x, x')^2 / (var(x) + s2 s_y^2)."""
    for gp, Z, X in cases:
        r = posterior(gp, X)
        sy2 = r["y_std"] ** 2
        for i in (0, 7):
            after = posterior(conditioned_on_one_more(gp, Z, X[i]), X)["raw_variance"]
            want = r["raw_variance"] - r["covariance"][i] ** 2 / (r["raw_variance"][i] + gp.noise * sy2)
            assert np.abs(after - want).max() <= 1e-11 * sy2, (i, np.abs(after - want).max() / sy2)


def test_posterior_symbols_declared_and_exported(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    for name in ("pcabo_gp_posterior", "pcabo_batch_gp_posterior"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in native.EXPORTS
        assert hasattr(native.LIB, name)
    assert re.search(r"PCABO_POST_OBS_NOISE\s*=\s*1\b", header) and native.POST_OBS_NOISE == 1
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2


def test_posterior_methods_exist_and_refuse_without_a_run(native):
    from Algorithms import PCA_BO, Vanilla_BO
    assert callable(native.Context.gp_posterior) and callable(native.Batch.gp_posterior)
    for cls in (PCA_BO, Vanilla_BO):
        opt = cls(budget=20, n_DoE=10, random_seed=1)
        with pytest.raises(RuntimeError):
            opt.posterior(np.zeros((3, 4)))
