"""The GP fit with one lengthscale per input (ARD), host side: the restatement of tests/ard_reference.py against central
differences and against the scalar restatement, the folding of the lengthscales into the Normalize ranges on the oracle, the margin
the ARD reference fit has over the scalar one, and the surface (keywords, command line, C symbols).

The device (tests/test_gpu_ard.py) is checked against the same restatement.  Parity with BoTorch / GPyTorch is not pinned, as for
the scalar fit.
"""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import pcabo_oracle as O
from ard_reference import EVAL_ONLY_STATE, FIT_STATES, RHO_MIN, ArdFit, ard_loss, ard_state, fitted_gp, softplus, theta0
from test_gp_fit_cpu import RestatedFit, restated_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _theta(seed, k):
    rng = np.random.default_rng(seed)
    return np.r_[0.05, 0.3, rng.uniform(-1.5, 2.0, size=k)]


@pytest.mark.parametrize("seed,n,k", [(1, 24, 2), (2, 40, 5), (3, 30, 9)])
def test_ard_gradient_matches_central_differences(seed, n, k):
    torch.set_num_threads(1)
    fit = ArdFit(*ard_state(seed, n, k))
    lin = _theta(seed, k)
    lin[2 + seed % k] = 25.0                                 # softplus's linear branch
    for theta in (theta0(k), _theta(seed, k), np.r_[1e-4, -0.2, _theta(seed, k)[2:]], lin):
        _, g = fit.value_and_grad(theta)
        for i in range(2 + k):
            h = 1e-5 * theta[0] if i == 0 else 1e-6          # (the noise: a step relative to its value, inside its domain)
            tp, tm = theta.copy(), theta.copy()
            tp[i] += h
            tm[i] -= h
            fd = (fit.value_and_grad(tp)[0] - fit.value_and_grad(tm)[0]) / (2.0 * h)
            assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])), (seed, theta, i, fd, g[i])


@pytest.mark.parametrize("seed,n,k", [EVAL_ONLY_STATE] + FIT_STATES[:2])
def test_equal_rho_is_the_scalar_restatement(seed, n, k):
    torch.set_num_threads(1)
    Z, y = ard_state(seed, n, k)
    ard, scalar = ArdFit(Z, y), RestatedFit(Z, y)
    for s2, c, rho in ((np.exp(-5.0), 0.0, 0.0), (1e-4, 0.3, -0.5), (0.05, -0.2, 0.8)):
        la, ga = ard.value_and_grad(np.r_[s2, c, np.full(k, rho)])
        ls, gs = scalar.value_and_grad((s2, c, rho))
        assert abs(la - ls) <= 1e-12 * max(1.0, abs(ls))
        assert np.abs(ga[:2] - gs[:2]).max() <= 1e-10 * max(1.0, np.abs(gs).max())
        assert abs(ga[2:].sum() - gs[2]) <= 1e-10 * max(1.0, abs(gs[2]))
        assert np.allclose(ard.term_scales(np.r_[s2, c, np.full(k, rho)])[2:].sum(), scalar.term_scales((s2, c, rho))[2], rtol=1e-10)
    th = torch.tensor(np.r_[0.05, -0.2, np.full(k, 0.8)])
    assert float(ard_loss(ard.Zn, ard.ys, th)) == pytest.approx(float(restated_loss(ard.Zn, ard.ys, th[:3])), rel=1e-12)


def test_folded_bounds_with_lengthscale_one_are_the_vector_lengthscale():
    """What the device does: Normalize ranges (hi - lo) l_c and lengthscale 1 instead of a vector lengthscale."""
    torch.set_num_threads(1)
    seed, n, k = FIT_STATES[1]
    Z, y = ard_state(seed, n, k)
    ls = softplus(np.r_[0.3, -1.0, 3.0, 6.0, 25.0])
    hp = {"lengthscales": ls, "noise": 0.01, "mean_constant": 0.2}
    vec = fitted_gp(Z, y, hp)
    nb = O.normalize_bounds(Z)
    folded_nb = np.vstack([nb[0], nb[0] + (nb[1] - nb[0]) * ls])
    folded = fitted_gp(Z, y, {**hp, "lengthscales": np.ones(k)}, norm_bounds=folded_nb)
    box = O.acq_bounds(Z)
    X = np.random.default_rng(5).uniform(box[0], box[1], size=(64, k))
    best_f = float(y.min())
    v, g = O.Acquisition(vec, best_f, False).value_and_grad(X)
    fv, fg = O.Acquisition(folded, best_f, False).value_and_grad(X)
    assert np.abs(v - fv).max() <= 1e-10 * max(1.0, np.abs(v).max())
    assert np.abs(g - fg).max() <= 1e-10 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("seed,n,k", FIT_STATES)
def test_reference_ard_fit_beats_the_scalar_fit(seed, n, k):
    torch.set_num_threads(2)
    Z, y = ard_state(seed, n, k)
    ard, scalar = ArdFit(Z, y).fit(), RestatedFit(Z, y).fit()
    assert ard.status == 0 and scalar.status == 0, (ard.message, scalar.message)
    assert ard.fun <= scalar.fun - 0.5, (ard.fun, scalar.fun)           # measured gaps: 0.68, 1.23, 1.44
    ls = softplus(ard.x[2:])
    assert ls[2:].min() > 5.0 * ls[:2].max(), ls                           # the inputs y does not depend on are switched off


def test_reference_fit_with_the_device_fits_bound_on_rho():
    """The device fit bounds every rho_c below (DESIGN.md "ARD lengthscales"); ArdFit.fit(rho_min=RHO_MIN) restates that.  A bound
    no trial step touches leaves scipy's path alone, bit for bit; the state whose unbounded fit leaves the domain ends with status 0."""
    torch.set_num_threads(2)
    src = open(os.path.join(ROOT, "para-ortho-pca-bo_amd", "csrc", "host_side.h"), encoding="utf-8").read()
    assert float(re.search(r"FIT_ARD_RHO_MIN = (-[0-9.]+);", src).group(1)) == RHO_MIN
    seed, n, k = FIT_STATES[0]
    fit = ArdFit(*ard_state(seed, n, k))
    free, bounded = fit.fit(), fit.fit(rho_min=RHO_MIN)
    assert free.x.tobytes() == bounded.x.tobytes() and free.nfev == bounded.nfev and bounded.status == 0
    fit = ArdFit(*ard_state(*EVAL_ONLY_STATE))
    with pytest.raises(RuntimeError):                                      # rho_c = -inf .. : not positive definite
        fit.fit()
    bounded = fit.fit(rho_min=RHO_MIN)
    assert bounded.status == 0 and bounded.x[2:].min() > RHO_MIN, (bounded.message, bounded.x)
    ls = softplus(bounded.x[2:])
    assert ls[2:].min() > 5.0 * ls[:2].max(), ls


def test_ard_keyword_refusals(native):
    from Algorithms import PCA_BO, Vanilla_BO, ExperimentRunner
    from pcabo.batchrun import BatchedPCABO, BatchedVanillaBO
    for cls in (PCA_BO, Vanilla_BO):
        with pytest.raises(ValueError, match="fit_gp"):
            cls(budget=20, n_DoE=10, ard=True)
    runner = dict(algorithms=["pca"], dimensions=[10], problem_ids=[15], num_runs=30, progress=False)
    with pytest.raises(ValueError, match="PCA_BO / Vanilla_BO"):
        ExperimentRunner(batched=30, fit_gp=False, batched_fit_gp=True, ard=True, **runner)
    with pytest.raises(ValueError, match="fit_gp"):
        ExperimentRunner(ard=True, **runner)
    assert ExperimentRunner(fit_gp=True, ard=True, **runner).ard is True
    assert ExperimentRunner(fit_gp=True, **runner).ard is False
    for cls in (BatchedPCABO, BatchedVanillaBO):
        with pytest.raises(ValueError, match="PCA_BO / Vanilla_BO"):
            cls([], [], budget=20, n_DoE=10, fit_gp=True, ard=True)


def test_main_parses_ard(native):
    spec = importlib.util.spec_from_file_location("pcabo_main_cli_ard", os.path.join(ROOT, "para-ortho-pca-bo_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    saved = os.environ.get("GPU_MAX_HW_QUEUES")          # (main.py sets a default for the processes it drives)
    try:
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            os.environ.pop("GPU_MAX_HW_QUEUES", None)
        else:
            os.environ["GPU_MAX_HW_QUEUES"] = saved
    a = mod.parse_arguments(["--fit_gp", "--ard"])
    assert a.ard is True and a.fit_gp is True
    assert mod.parse_arguments(["--fit_gp"]).ard is False


def test_ard_symbols_declared_and_exported(native):
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    for name in ("pcabo_gp_mll_ard", "pcabo_gp_fit_ard"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in native.EXPORTS
        assert hasattr(native.LIB, name)
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2
