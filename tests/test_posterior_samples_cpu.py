"""GP posterior samples (pcabo_gp_posterior_sample / pcabo_batch_gp_posterior_sample), host side: the long-double reference of
tests/posterior_samples_reference.py against torch's own Cholesky and rsample formula, the conditioning of the inputs the device's
forward test uses, the surface from the header to the optimiser classes, and the argument rules that need no device.  The device
results are checked in tests/test_gpu_posterior_samples.py."""
import os
import re

import numpy as np
import pytest
import torch

import pcabo_oracle as O
from posterior_samples_reference import SHAPES, base_samples, nasty_queries, plain_queries, posterior_samples, state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_matches_torch_on_the_forward_inputs():
    """Both are exact algorithms, so on well-conditioned inputs they agree to rounding: 1e-10 s_y.  The inputs are those of the
    device's forward test - every row of SHAPES with plain queries and observation noise on - and their cond_2 is at most 1e6."""
    torch.set_num_threads(4)
    for shape in SHAPES:
        n, k, q, S, kernel = shape[:5]
        Z, y, nb = state(shape)
        X = plain_queries(Z, q, n + q)
        base = base_samples(q, S)
        ref = posterior_samples(O.ExactGP(Z, y, nb, kernel=kernel), X, base, observation_noise=True)
        assert ref["jitter"] == 0.0 and ref["cond"] <= 1e6, (shape, ref["jitter"], ref["cond"])
        scale_tril = torch.linalg.cholesky(torch.from_numpy(ref["covariance"]))
        want = torch.from_numpy(ref["mean"]) + torch.from_numpy(base) @ scale_tril.mT          # loc + eps @ scale_tril^T
        err = np.abs(np.asarray(ref["samples"], dtype=np.float64) - want.numpy()).max() / ref["y_std"]
        assert err <= 1e-10, (shape, err)
        centred = posterior_samples(O.ExactGP(Z, y, nb, kernel=kernel), X, base, observation_noise=True, centred=True)
        assert np.abs(np.asarray(centred["samples"] + ref["mean"] - ref["samples"], dtype=np.float64)).max() <= 1e-14 * max(
            1.0, np.abs(ref["mean"]).max())


def test_reference_ladder_climbs_on_a_singular_covariance():
    shape = SHAPES[1]
    Z, y, nb = state(shape)
    X = nasty_queries(Z, shape[2], 1)
    ref = posterior_samples(O.ExactGP(Z, y, nb), X, np.eye(shape[2]), centred=True)           # an exact duplicate row, no noise
    assert ref["jitter"] in (1e-8, 1e-7, 1e-6)
    L = ref["factor"]
    A = np.asarray(ref["covariance"], dtype=np.longdouble) + np.longdouble(ref["jitter"]) * np.longdouble(ref["y_std"]) ** 2 * np.eye(shape[2])
    assert np.array_equal(ref["samples"].T, L)                                                # base = I reads the factor
    # (the factorisation reads the lower triangle; the oracle's cov is symmetric to float64 rounding only)
    assert np.abs(np.asarray(np.tril(L @ L.T - A), dtype=np.float64)).max() <= 64 * 2.0 ** -63 * ref["y_std"] ** 2


def test_sample_symbols_declared_and_exported(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    for name in ("pcabo_gp_posterior_sample", "pcabo_batch_gp_posterior_sample"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in native.EXPORTS
        assert hasattr(native.LIB, name)
    assert re.search(r"PCABO_POST_CENTRED\s*=\s*2\b", header) and native.POST_CENTRED == 2
    assert re.search(r"#define\s+PCABO_POST_MAX_SAMPLES\s+1024\b", header) and native.POST_MAX_SAMPLES == 1024
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2
    assert re.search(r"#define\s+PCABO_ABI_VERSION\s+2\b", open(os.path.join(ROOT, "para-ortho-pca-bo_amd", "csrc", "pcabo_api.hip")).read())


def test_base_rules_need_no_device(native):
    with pytest.raises(ValueError):
        native.sample_base(5)                                                     # neither
    with pytest.raises(ValueError):
        native.sample_base(5, n_samples=3, base_samples=np.zeros((3, 5)))         # both
    for bad in (np.zeros((3, 4)), np.zeros(5), np.zeros((0, 5)), np.zeros((2, 3, 5))):
        with pytest.raises(ValueError):
            native.sample_base(5, base_samples=bad)                               # not S x q
    with pytest.raises(ValueError):
        native.sample_base(5, n_samples=0)
    given = np.arange(10.0).reshape(2, 5)
    assert np.array_equal(native.sample_base(5, base_samples=given), given)
    np.random.seed(123)
    torch.manual_seed(123)
    s_np, s_torch = np.random.get_state(), torch.random.get_rng_state().clone()
    a, b = native.sample_base(7, n_samples=4, seed=11), native.sample_base(7, n_samples=4, seed=11)
    assert a.shape == (4, 7) and a.dtype == np.float64 and a.tobytes() == b.tobytes()
    assert a.tobytes() == np.random.default_rng(11).standard_normal((4, 7)).tobytes()
    assert a.tobytes() != native.sample_base(7, n_samples=4, seed=12).tobytes()
    native.sample_base(7, n_samples=4)                                            # unseeded: fresh entropy, still no global state
    now = np.random.get_state()
    assert s_np[0] == now[0] and s_np[1].tobytes() == now[1].tobytes() and s_np[2:] == now[2:]
    assert s_torch.numpy().tobytes() == torch.random.get_rng_state().numpy().tobytes()


def test_sample_methods_exist_and_refuse_without_a_run(native):
    from Algorithms import PCA_BO, Vanilla_BO
    assert callable(native.Context.gp_posterior_samples) and callable(native.Batch.gp_posterior_samples)
    for cls in (PCA_BO, Vanilla_BO):
        opt = cls(budget=20, n_DoE=10, random_seed=1)
        with pytest.raises(RuntimeError):
            opt.posterior_samples(np.zeros((3, 4)), n_samples=2, seed=0)
