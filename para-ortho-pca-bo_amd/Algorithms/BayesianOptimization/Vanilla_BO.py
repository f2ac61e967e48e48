"""Plain (full-dimensional) Bayesian optimisation on MI355X.

Same call surface as the reference's `Vanilla_BO`
(/root/reference/Algorithms/BayesianOptimization/Vanilla_BO.py:39-301).  It is the PCA_BO loop without the PCA:
the exact GP lives on the raw d-dimensional points (the reference disables `Normalize` there,
Vanilla_BO.py:188-194, so the kernel sees raw coordinates), the acquisition is optimised inside the problem's
box (Vanilla_BO.py:206-213) and there is no out-of-bounds rule.  It runs on the same libpcabo kernels:

    SingleTaskGP(...) + lazy Gram/Cholesky (:166-196, :206)   Context.gp_condition(Z = X, identity Normalize bounds)
    optimize_acqf (:206-213)                                  pcabo.acqopt.optimize_acqf (device scoring + L-BFGS-B)

The loop, the keywords, the model queries and the acquisition-name handling are DeviceBayesianOptimizer's, shared with PCA_BO.
"""
from __future__ import annotations

from time import perf_counter

import numpy as np

from pcabo import _native
from pcabo import acqopt as _acqopt
from pcabo import initializers as _init
from .DeviceBayesianOptimizer import DeviceBayesianOptimizer, LENGTHSCALE, NOISE, fit_gp_hyperparameters


class Vanilla_BO(DeviceBayesianOptimizer):
    TIME_PROFILES = ["SingleTaskGP", "optimize_acqf"]
    ODD_NAME = "Oddly defined name {name}"
    FINAL_LINE = "Optimisation Process finalized!"

    def __str__(self):
        return "This is an instance of a Vanilla BO Optimizer"

    def _open_run(self, problem) -> None:
        d = self.dimension
        self.__identity = np.vstack([np.zeros(d), np.ones(d)])          # Normalize is switched off in the reference
        self.__box = np.ascontiguousarray(self.bounds.T, dtype=np.float64)   # 2 x d search box

    def _condition_model(self, **kwargs) -> None:
        self._initialise_model(**kwargs)

    def _observe(self, problem, candidate) -> float:
        x = np.asarray(candidate, dtype=np.float64).ravel()
        self.x_evals.append(x)
        return problem(x)

    def _initialise_model(self, **kwargs):
        X = np.array(self.x_evals, dtype=np.float64).reshape((-1, self.dimension))
        y = np.array(self.f_evals, dtype=np.float64)
        start = perf_counter()
        if self._fit_gp:
            self.gp_hyperparameters = fit_gp_hyperparameters(self._ctx, y, Z=X, norm_bounds=self.__identity, ard=self._ard)
            self.timing_logs["SingleTaskGP"].append(perf_counter() - start)
            return
        self._ctx.gp_condition(y, Z=X, norm_bounds=self.__identity, lengthscale=LENGTHSCALE, noise=NOISE,
                               kernel=_native.KERNEL_MATERN52, wait=False)
        self.timing_logs["SingleTaskGP"].append(perf_counter() - start)

    def optimize_acqf_and_get_observation(self) -> np.ndarray:
        ctx, cfg, acq = self._ctx, self._torch_config, self.acquisition_function
        start = perf_counter()
        engine = _init.scrambled_sobol_engine(self.dimension)      # built and drawn while the device conditions the GP
        raw = _init.draw_sobol(self.__box, cfg["RAW_SAMPLES"], engine)
        raw_vals = None                    # (fit_gp: the GP is conditioned already, the optimiser scores the raw samples)
        one_call = self._scores_in_one_call(acq)   # (then the optimiser's one call waits for the conditioning and scores)
        if not self._fit_gp and not one_call:
            t0 = perf_counter()            # the raw samples are scored right behind the conditioning: one wait for both
            raw_vals = ctx.gp_wait_eval(raw, acq.device_scalar, acq.maximize, acq.acq_code)
            self.phase_breakdown["raw_eval"] = self.phase_breakdown.get("raw_eval", 0.0) + perf_counter() - t0
        new_x, infos = _acqopt.propose(
            ctx, self.__box, acq.device_scalar, acq.maximize, acq.acq_code, cfg["NUM_RESTARTS"], cfg["RAW_SAMPLES"], 5, 200,
            q_eff=self._q_eff(), strategy=self._q_strategy, f_evals=self.f_evals, raw=raw, raw_vals=raw_vals, breakdown=self.phase_breakdown,
            trace=self.trace[-1] if self._record_trace else None, one_call=one_call)
        self.timing_logs["optimize_acqf"].append(perf_counter() - start)
        self.lbfgsb_info.extend(infos)
        return new_x
