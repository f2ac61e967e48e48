"""One Bayesian-optimisation run on the device: what `PCA_BO` and `Vanilla_BO` have in common.

`DeviceBayesianOptimizer` stands between `AbstractBayesianOptimizer` (the initial design and the bookkeeping, as in the reference)
and the two optimisers.  It owns the keywords both take, the run's libpcabo context, the loop (`__call__` and its three pieces
`_start` / `_bo_iteration` / `_finish`), the queries of the iteration's model (`posterior`, `posterior_samples`, `loo`, `fantasy`)
and the acquisition-name plumbing of the reference (PCA_BO.py:643-720, Vanilla_BO.py:225-301).  A subclass fills in

    _condition_model(**kwargs)              from the evaluated points to this iteration's GP in the context (enqueued or conditioned)
    optimize_acqf_and_get_observation()     the iteration's candidates, in model space
    _observe(problem, candidate)            appends the candidate's point to x_evals, returns its objective value
    _open_run(problem) / _close_run()       its own set-up behind the context's / its own tear-down in front of the shared one
    _model_ready() / _to_model_space(X)     for the model queries: is this iteration's GP conditioned, and where does X lie in it

and the two class attributes that carry the reference's per-class wording (ODD_NAME, FINAL_LINE).
"""
from __future__ import annotations

import os
import warnings
from abc import abstractmethod
from contextlib import contextmanager
from typing import Callable, Optional, Union

import numpy as np

from pcabo import _native
from pcabo import acqopt as _acqopt
from pcabo.acqopt import ALLOWED_ACQUISITION_FUNCTION_STRINGS, ALLOWED_SHORTHAND_ACQUISITION_FUNCTION_STRINGS  # noqa: F401
from pcabo.gcguard import RunGuard
from .AbstractBayesianOptimizer import AbstractBayesianOptimizer

# Model constants of the never-trained SingleTaskGP(MaternKernel(2.5)).
LENGTHSCALE = 0.6931471805599453     # softplus(0)
NOISE = 0.006737946999085467         # exp(-5), mode of the LogNormal(-4, 1) noise prior


def checked_ard(ard, fit_gp) -> bool:
    """The `ard` keyword of PCA_BO / Vanilla_BO: one lengthscale per input is a mode of the fit."""
    if ard and not fit_gp:
        raise ValueError("ard=True fits one lengthscale per input: it needs fit_gp=True")
    return bool(ard)


def fit_gp_hyperparameters(ctx, y, Z=None, norm_bounds=None, ard=False) -> dict:
    """fit_gpytorch_mll(ExactMarginalLogLikelihood(...)) of a freshly built model, on the device (Context.gp_fit; ard: one
    lengthscale per input, Context.gp_fit_ard); like botorch, a fit that does not converge keeps its last iterate and warns."""
    if ard:
        hp = ctx.gp_fit_ard(y, Z=Z, norm_bounds=norm_bounds)
    else:
        hp = ctx.gp_fit(y, Z=Z, norm_bounds=norm_bounds, kernel=_native.KERNEL_MATERN52)
    if hp["warnflag"] != 0:
        warnings.warn(f"GP hyperparameter fit did not converge (warnflag {hp['warnflag']}, task {hp['task']}); keeping the last "
                      "accepted iterate", RuntimeWarning)
    return hp


class AnalyticAcquisitionFunction:
    """Descriptor of the acquisition the device kernels evaluate (stands in for botorch's class)."""
    acq_code = _native.ACQ_LOG_EI

    def __init__(self, model=None, best_f: float = 0.0, maximize: bool = True):
        self.model, self.best_f, self.maximize = model, best_f, maximize

    @property
    def device_scalar(self) -> float:
        """The one scalar the device takes with `acq_code` (the `best_f` slot of the C ABI): best_f here, kappa for UCB."""
        return self.best_f


class LogExpectedImprovement(AnalyticAcquisitionFunction):
    acq_code = _native.ACQ_LOG_EI


class ProbabilityOfImprovement(AnalyticAcquisitionFunction):
    acq_code = _native.ACQ_PI


class UpperConfidenceBound(AnalyticAcquisitionFunction):
    """botorch's signature: UpperConfidenceBound(model, beta, maximize=True); value = +-mean + sqrt(beta) sigma.
    The reference constructs its acquisition with `best_f=` (PCA_BO.py:199-203), which that signature does not accept: the
    first BO iteration raises TypeError.  That behaviour is kept; the optimisers' `ucb_beta` keyword (not in the reference)
    is what constructs it the way botorch accepts."""
    acq_code = _native.ACQ_UCB

    def __init__(self, model=None, beta=None, maximize: bool = True, **kwargs):
        if kwargs or beta is None:
            raise TypeError("UpperConfidenceBound.__init__() got an unexpected keyword argument 'best_f'")
        super().__init__(model, 0.0, maximize)
        self.beta = beta
        self.kappa = _acqopt.ucb_kappa(beta)       # float32 sqrt like botorch's beta tensor; the device gets kappa, never beta

    @property
    def device_scalar(self) -> float:
        return self.kappa


_ACQUISITION_CLASSES = dict(zip(ALLOWED_ACQUISITION_FUNCTION_STRINGS,
                                (LogExpectedImprovement, ProbabilityOfImprovement, UpperConfidenceBound)))


class DeviceBayesianOptimizer(AbstractBayesianOptimizer):
    ODD_NAME = "Oddly defined name"                      # ValueError of the name setter; `{name}` stands for the name given
    FINAL_LINE = "Optimization Process finalized!"       # the last verbose line of a run

    def __init__(self, budget: int, n_DoE: int = 0, acquisition_function: str = "expected_improvement",
                 random_seed: int = 43, **kwargs):
        self._device = int(kwargs.pop("device", 0))
        self._record_trace = bool(kwargs.pop("record_trace", False))
        # torch_threads: torch's intra-op threads are capped for the duration of a run (None = left alone); gc_freeze: the
        # interpreter's cyclic collector is kept away from the loop (0.3-0.45 ms per iteration otherwise).  Both: pcabo/gcguard.py
        self._guard = RunGuard(kwargs.pop("torch_threads", 4), kwargs.pop("gc_freeze", True))
        # resident=False: one launch per acquisition evaluation instead of the resident kernel of pcabo_optimize_acqf
        # (PCABO_OPT_RESIDENT; same arithmetic - the tests compare whole runs bit for bit)
        self._resident = bool(kwargs.pop("resident", True))
        # one_call=False: scoring of the raw samples, initial pick and optimiser stay three calls with torch's pick between them;
        # True (default; the environment's PCABO_ONE_CALL=0 turns the default off): one native call (pcabo_propose_acqf), which
        # also ends the conditioning in flight - same arithmetic, same generator stream (the tests compare whole runs)
        self._one_call = bool(kwargs.pop("one_call", _acqopt.one_call_default()))
        # fantasy_points: room for that many points behind the budget in the run's context, for fantasy() (0: the context holds the
        # budget and fantasy() fits only while n + its points <= budget)
        self._fantasy_points = int(kwargs.pop("fantasy_points", 0))
        if self._fantasy_points < 0:
            raise ValueError("fantasy_points must be >= 0")
        # fit_gp=True (not in the reference, which never trains its GP): every iteration fits (noise, mean constant, lengthscale)
        # by the marginal likelihood from the model's initial values before the acquisition (Context.gp_fit, DESIGN.md "GP
        # hyperparameter fit").  False keeps the reference's fixed hyperparameters.
        self._fit_gp = bool(kwargs.pop("fit_gp", False))
        # ard=True (needs fit_gp=True): the fit trains one lengthscale per input of the model - per principal component in PCA_BO
        # (Context.gp_fit_ard, DESIGN.md "ARD lengthscales"): Normalize stretches every component to the same unit box, and a single
        # lengthscale cannot tell them apart
        self._ard = checked_ard(kwargs.pop("ard", False), self._fit_gp)
        self.gp_hyperparameters = None     # fit_gp=True: the last fit's result (Context.gp_fit / gp_fit_ard), None otherwise
        # ucb_beta (not in the reference, whose UCB cannot run): with acquisition_function "UCB" every iteration builds
        # UpperConfidenceBound(model, beta=ucb_beta, maximize=...), botorch's own signature.  None keeps the reference's TypeError.
        self._ucb_beta = _acqopt.checked_ucb_beta(kwargs.pop("ucb_beta", None), acquisition_function)
        # q, q_strategy (not in the reference, whose BATCH_SIZE never reaches optimize_acqf): every iteration proposes q candidates,
        # one after the other on a model that takes each pending point in - at its own mean ("kriging_believer") or at the min / mean /
        # max of the values seen ("constant_liar_*") - and evaluates them in that order (pcabo.acqopt.propose).
        # The last iteration proposes what the budget leaves.  q=1 is the reference's loop.
        self._q, self._q_strategy = _acqopt.checked_q(kwargs.pop("q", 1), kwargs.pop("q_strategy", "kriging_believer"))
        super().__init__(budget, n_DoE, **kwargs)
        self.random_seed = random_seed
        smoke_test = os.environ.get("SMOKE_TEST")
        self._torch_config = {
            "device": f"hip:{self._device}",
            "dtype": np.float64,
            "SMOKE_TEST": smoke_test,
            "BATCH_SIZE": 3 if not smoke_test else 2,
            "NUM_RESTARTS": 10 if not smoke_test else 2,
            "RAW_SAMPLES": 512 if not smoke_test else 32,
        }
        self._acq_func_class = None
        self._acq_func = None
        self.acquisition_function_name = acquisition_function
        self._ctx: Optional[_native.Context] = None
        self.lbfgsb_info = []          # per iteration: (iterations, evaluations, warnflag, task) per restart group
        self.trace = []                # record_trace=True: per iteration RNG states, restart candidates/values
        self.phase_breakdown = {}      # seconds inside optimize_acqf, per phase

    # ---------------------------------------------------------------------------------------------
    def __call__(self, problem: Union[Callable, object], dim: Optional[int] = -1,
                 bounds: Optional[np.ndarray] = None, **kwargs) -> None:
        try:
            self._start(problem, dim, bounds, **kwargs)      # inside the try: whatever it switched on is switched off again
            for _ in range(self.budget - self.n_DoE):
                if self.number_of_function_evaluations >= self.budget:
                    break
                self._bo_iteration(problem, **kwargs)
        finally:
            self._finish()

    # The three pieces of `__call__`, exposed so that a driver (bench.py, the sharded runner) can time or
    # interleave single BO iterations; together they are exactly the reference's loop (PCA_BO.py:140-310).
    def _start(self, problem, dim=-1, bounds=None, **kwargs) -> None:
        self._guard.enter()
        self.impose_random_seed()
        AbstractBayesianOptimizer.__call__(self, problem, dim, bounds, **kwargs)
        if self._pbar is not None:
            self._pbar.update(self.n_DoE)
        self._ctx = _native.Context(max_n=self.budget + self._fantasy_points, max_d=self.dimension,
                                    max_q=max(self._torch_config["RAW_SAMPLES"], 16), device=self._device)
        if not self._resident:
            self._ctx.set_option(_native.OPT_RESIDENT, 0)
        self._open_run(problem)

    def _bo_iteration(self, problem, **kwargs) -> None:
        if self._record_trace:
            import torch
            self.trace.append({"n": len(self.f_evals), "numpy_state": np.random.get_state(),
                               "torch_state": torch.get_rng_state(), "best_f": self.current_best})
        self._condition_model(**kwargs)
        self._ctx.match_best_f_dtype(self.current_best)      # float32 like torch.as_tensor(python float), or all 64 bits
        if self._ucb_beta is not None:
            self.acquisition_function = self.acquisition_function_class(
                model=self._ctx, beta=self._ucb_beta, maximize=self.maximization)
        else:
            self.acquisition_function = self.acquisition_function_class(
                model=self._ctx, best_f=self.current_best, maximize=self.maximization)
        for candidate in self.optimize_acqf_and_get_observation():
            if self.number_of_function_evaluations >= self.budget:
                break
            new_f = self._observe(problem, candidate)
            if self._pbar is not None:
                self._pbar.update(1)
            self.f_evals.append(new_f)
            self.number_of_function_evaluations += 1
        self.assign_new_best()
        if self.verbose:
            print(f"Evaluations: {self.number_of_function_evaluations}/{self.budget}",
                  f"Best: x:{self.x_evals[self.current_best_index]} y:{self.current_best}", flush=True)

    def _finish(self) -> None:
        self._close_run()
        self._guard.leave()
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
        if self.verbose:
            print(self.FINAL_LINE)
        self.restore_random_states()

    def _scores_in_one_call(self, acq) -> bool:
        """Does pcabo.acqopt.optimize_acqf score this iteration's raw samples itself (its one native call, which also ends a
        conditioning in flight)?  Then the optimiser hands it `raw` alone."""
        cfg = self._torch_config
        return self._one_call and _acqopt.one_call_applies(self._ctx, acq.acq_code, cfg["NUM_RESTARTS"], cfg["RAW_SAMPLES"])

    def _q_eff(self) -> int:
        """Candidates of the current iteration: q, or what the budget leaves."""
        return max(1, min(self._q, self.budget - len(self.f_evals)))

    def assign_new_best(self):
        super().assign_new_best()

    # ---- what a subclass fills in -----------------------------------------------------------------
    @abstractmethod
    def _condition_model(self, **kwargs) -> None:
        """From the evaluated points to this iteration's GP in the context."""

    @abstractmethod
    def optimize_acqf_and_get_observation(self) -> np.ndarray:
        """The iteration's candidates (`_q_eff()` of them), one row each, in the space of the model."""

    @abstractmethod
    def _observe(self, problem, candidate) -> float:
        """Append the candidate's point to x_evals and return its objective value."""

    def _open_run(self, problem) -> None:
        """Set-up of the subclass, the context is open."""

    def _close_run(self) -> None:
        """Tear-down of the subclass, in front of the shared one; also called after a start that failed."""

    def _model_ready(self) -> bool:
        """Is this iteration's GP conditioned?  (A context that is not refuses the query itself: PcaboError, a RuntimeError.)"""
        return True

    def _to_model_space(self, X: np.ndarray) -> np.ndarray:
        """X (m x d, original space) as the model's input."""
        return X

    # ---- what the model predicts (the reference's model.posterior(test_points), visualization_utils.py:458-461) -------
    def _model_input(self, query: str, X=None):
        """The check in front of every model query, then X (if any) as m x d in model space."""
        if self._ctx is None or not self._model_ready():
            raise RuntimeError(f"{query}: no run is open, or the model of the current iteration is not conditioned yet")
        if X is not None:
            return self._to_model_space(np.asarray(X, dtype=np.float64).reshape(-1, self.dimension))

    def posterior(self, X, observation_noise: bool = False, covariance: bool = False) -> dict:
        """Posterior of the current iteration's GP at X (m x d, original space): {"mean", "variance"[, "covariance"]}
        (Context.gp_posterior).  PCA_BO maps X into the reduced space on the host with this iteration's centring and components.
        RuntimeError when no run is open or the iteration's model is not conditioned yet.  Leaves the run's trajectory alone."""
        Z = self._model_input("posterior", X)
        return self._ctx.gp_posterior(Z, observation_noise, covariance)

    def posterior_samples(self, X, n_samples=1, seed=None, base_samples=None, observation_noise: bool = False,
                          centred: bool = False) -> dict:
        """Joint draws of the current iteration's GP at X (m x d, original space): {"samples" (S, m), "mean" (m,), "jitter"}
        (Context.gp_posterior_samples).  The base is n_samples rows from a generator of its own seeded with `seed`, or the caller's
        base_samples (S x m), which replace n_samples.  Mapping and RuntimeErrors as posterior(); leaves the run's trajectory alone."""
        Z = self._model_input("posterior_samples", X)
        return self._ctx.gp_posterior_samples(Z, None if base_samples is not None else n_samples, base_samples, seed,
                                              observation_noise, centred)

    def loo(self) -> dict:
        """Leave-one-out predictions of the current iteration's GP at its own data: {"mean", "variance", "z", "lpd"} with one entry
        per evaluated point, in evaluation order, and "lpd_sum" (Context.gp_loo).  RuntimeErrors as posterior().  Leaves the run's
        trajectory alone."""
        self._model_input("loo")
        return self._ctx.gp_loo()

    @contextmanager
    def fantasy(self, X, y=None):
        """Inside the `with` body the current iteration's GP also holds the points X (m x d, original space, mapped like posterior())
        with values y (objective units; None: believer mode, every point takes the model's own mean there): transforms and
        hyperparameters held, only the data grow (Context.gp_extend).  posterior(), posterior_samples() and loo() see that model -
        loo() then has m more entries.  On exit the points are taken back, also when the body raises, and the run goes on bit for
        bit as without the visit.  The context must have room for n + m points: construct the optimiser with fantasy_points=m (the library
        refuses the call otherwise: PcaboError, a RuntimeError).  RuntimeErrors as posterior()."""
        Z = self._model_input("fantasy", X)
        n0 = self._ctx.n
        self._ctx.gp_extend(Z, y)
        try:
            yield self
        finally:
            self._ctx.gp_truncate(n0)

    # ---- the run's context, configuration and acquisition (reference PCA_BO.py:643-720) -----------
    @property
    def device_context(self):
        """The live libpcabo context of a run in progress (profiling hooks); None outside a run."""
        return self._ctx

    @property
    def torch_config(self) -> dict:
        return self._torch_config

    @property
    def acquisition_function_name(self) -> str:
        return self._acquisition_function_name

    @acquisition_function_name.setter
    def acquisition_function_name(self, new_name: str) -> None:
        self._acquisition_function_name = _acqopt.acquisition_long_name(new_name, self.ODD_NAME)
        self.set_acquisition_function_subclass()

    def set_acquisition_function_subclass(self) -> None:
        if self._acquisition_function_name in _ACQUISITION_CLASSES:      # (the reference's if-chain: no match, no change)
            self._acq_func_class = _ACQUISITION_CLASSES[self._acquisition_function_name]

    @property
    def acquisition_function_class(self) -> Callable:
        return self._acq_func_class

    @property
    def acquisition_function(self) -> AnalyticAcquisitionFunction:
        return self._acq_func

    @acquisition_function.setter
    def acquisition_function(self, new_acquisition_function: AnalyticAcquisitionFunction) -> None:
        if issubclass(type(new_acquisition_function), AnalyticAcquisitionFunction):
            self._acq_func = new_acquisition_function
        else:
            raise AttributeError("Acquisition function does not inherit from 'AnalyticAcquisitionFunction'",
                                 name="acquisition_function", obj=self._acq_func)
