"""PCA-assisted Bayesian optimisation on MI355X.

Same call surface as the reference's `PCA_BO`
(/root/reference/Algorithms/BayesianOptimization/PCA_BO.py:48-720): constructor keywords,
`__call__(problem, dim, bounds)`, result attributes, `TIME_PROFILES`, acquisition-name handling and
error behaviour.  The four places where the reference hands arithmetic to sklearn / botorch /
gpytorch / scipy are calls into libpcabo.so (HIP kernels for gfx950) here:

    reference                                              this file -> C ABI (include/pcabo.h)
    _calculate_weights + PCA().fit/transform (:316-408)    Context.wpca            pcabo_wpca
    SingleTaskGP(...) + lazy Gram/Cholesky (:502-545)      Context.gp_condition    pcabo_gp_condition
    optimize_acqf raw-sample scoring (:607)                Context.acq_eval        pcabo_acq_eval
    optimize_acqf multi-start L-BFGS-B (:607-614)          Context.optimize_acqf   pcabo_optimize_acqf
    pca.inverse_transform (:427)                           Context.inverse_map     pcabo_inverse_map

What stays on the host is exactly what the reference does in Python: ranking with numpy's argsort
(:330-333), the noise draw from numpy's global RNG (:376), Sobol / multinomial draws from torch's
global CPU generator (botorch initialisers), the out-of-bounds rule (:248-263) and bookkeeping.
There is no CPU fallback: importing this module needs libpcabo.so, running it needs a HIP device.

The loop (`__call__`, `_start` / `_bo_iteration` / `_finish`), the keywords shared with Vanilla_BO, the model queries and the
acquisition-name handling are DeviceBayesianOptimizer's; this file holds what only the PCA-assisted run has.
"""
from __future__ import annotations

import warnings
from time import perf_counter

import numpy as np

from pcabo import _native
from pcabo import initializers as _init
from pcabo import acqopt as _acqopt
from .DeviceBayesianOptimizer import (  # noqa: F401  (re-exported: users and tests import these names from here)
    ALLOWED_ACQUISITION_FUNCTION_STRINGS, ALLOWED_SHORTHAND_ACQUISITION_FUNCTION_STRINGS, AnalyticAcquisitionFunction,
    DeviceBayesianOptimizer, LogExpectedImprovement, ProbabilityOfImprovement, UpperConfidenceBound, LENGTHSCALE, NOISE,
    checked_ard, fit_gp_hyperparameters)

OOB_PENALTY = 1000


class _FittedPCA:
    """Read-only view of the device wPCA result with sklearn's attribute names (reference: `self.pca`)."""

    def __init__(self, components, mean, evr, k):
        self.components_ = components[:k]
        self.mean_ = mean
        self.explained_variance_ratio_ = evr
        self.n_components_ = components.shape[0]

    def transform(self, X):
        X = np.asarray(X, dtype=float)
        return X @ self.components_.T - self.mean_.reshape(1, -1) @ self.components_.T

    def inverse_transform(self, Z):
        return np.asarray(Z, dtype=float) @ self.components_ + self.mean_


class PCA_BO(DeviceBayesianOptimizer):
    TIME_PROFILES = ["SingleTaskGP", "optimize_acqf", "pca"]

    def __init__(self, budget: int, n_DoE: int = 0, n_components: int = 0, var_threshold: float = 0.95,
                 acquisition_function: str = "expected_improvement", random_seed: int = 43,
                 visualize: bool = False, **kwargs):
        # prefetch_noise: draw the NEXT iteration's 1e-8 noise matrix (numpy's global RNG, PCA_BO.py:376) on a helper
        # thread while the acquisition optimiser runs inside the library.  The numbers are the same, but they leave the
        # global stream BEFORE the objective of this iteration is evaluated - harmless exactly when the objective does
        # not draw from numpy's global RNG.  None = automatic: on for the in-repo BBOB problems, off otherwise.
        self.__prefetch = kwargs.pop("prefetch_noise", None)
        self.__prefetch_on = False
        self.__noise_thread, self.__noise_pending = None, False
        self.__noise_req = self.__noise_res = None
        # acq_kernel: "latency" (default: per-query kernels, resident across the evaluations of an optimize call - the
        # fastest for ONE run) or "group" (the throughput kernel the batched driver uses; a run then takes, bit for bit,
        # the path it takes inside a batch - pcabo.batchrun)
        self.__acq_kernel = str(kwargs.pop("acq_kernel", "latency"))
        if self.__acq_kernel not in ("latency", "group"):
            raise ValueError("acq_kernel must be 'latency' or 'group'")
        # fused_enqueue=False: pcabo_wpca and pcabo_gp_condition_begin as two calls instead of ONE enqueue of rows A-H (the
        # tests compare the two; fit_gp=True takes the unfused wPCA -> fit path too); early_scoring / engine_guess likewise
        # switch the two host/device overlaps off
        self.__fused = bool(kwargs.pop("fused_enqueue", True))
        self.__early_scoring = bool(kwargs.pop("early_scoring", True))
        self.__speculate_engine = bool(kwargs.pop("engine_guess", True))
        super().__init__(budget, n_DoE, acquisition_function=acquisition_function, random_seed=random_seed, **kwargs)
        self.n_components = n_components
        self.var_threshold = var_threshold
        self.data_mean = None
        self.pca = None
        self.component_matrix = None
        self.explained_variance_ratio = None
        self.reduced_space_dim_num = None
        self.visualize = visualize
        if visualize:
            warnings.warn("visualize=True: the GIF visualiser of the reference is not part of the MI355X path; ignored.")
        self.__z_evals = []
        self.__gp_pending = False
        self.__engine_ready = None
        self.__X_buf, self.__X_rows = None, 0
        self.phase_breakdown = {"sobol": 0.0, "raw_eval": 0.0, "init_pick": 0.0, "lbfgsb": 0.0}   # inside optimize_acqf

    def __str__(self):
        return "This is an instance of a PCA-assisted BO Optimizer"

    # ---- what the shared loop (DeviceBayesianOptimizer) asks of this class ---------------------------
    def _open_run(self, problem) -> None:
        if self.__acq_kernel == "group":
            self._ctx.set_option(_native.OPT_GROUP_ACQ, 1)
        self.__X_buf, self.__X_rows = None, 0
        if self.__prefetch is None:
            from pcabo.bbob import BBOBProblem
            self.__prefetch_on = isinstance(getattr(problem, "_problem", problem), BBOBProblem)
        else:
            self.__prefetch_on = bool(self.__prefetch)
        if self._record_trace:             # the recorded per-iteration RNG state must be the one BEFORE the draw
            self.__prefetch_on = False

    def _close_run(self) -> None:
        self._stop_noise_worker()

    def _condition_model(self, **kwargs) -> None:
        self._transform_points_to_reduced_space()
        self._initialize_model(**kwargs)

    def _observe(self, problem, candidate) -> float:
        new_z = np.asarray(candidate).ravel()
        new_x = self._transform_point_to_original_space(new_z)
        outside = not np.all(new_x >= self.bounds[:, 0]) or not np.all(new_x <= self.bounds[:, 1])
        if outside and self.verbose:
            print(f"Warning: PCA transformed point {new_x} was out of bounds, clipping to boundary")
        self.x_evals.append(new_x)
        self.__z_evals.append(new_z)
        # out-of-box candidates are not evaluated; they cost budget and a fixed penalty (PCA_BO.py:260-263)
        new_f = (-OOB_PENALTY if self.maximization else OOB_PENALTY) if outside else problem(new_x)
        if self.verbose and ((self.maximization and new_f > self.current_best) or
                             (not self.maximization and new_f < self.current_best)):
            print(f"Found better solution: {new_f}")
            print(f"At point: {new_x}")
        return new_f

    def _model_ready(self) -> bool:
        return self.pca is not None and not self.__gp_pending

    def _to_model_space(self, X: np.ndarray) -> np.ndarray:
        return self.pca.transform(X - self.data_mean)

    # ---- row A (host part): ranks exactly as numpy gives them ------------------------------------
    def _calculate_ranks(self) -> np.ndarray:
        f = np.array(self.f_evals)
        return np.argsort(np.argsort(-f if self.maximization else f)) + 1

    def _calculate_weights(self) -> np.ndarray:
        pre = np.log(len(self.f_evals)) - np.log(self._calculate_ranks())
        return pre / pre.sum()

    # ---- rows A-C ---------------------------------------------------------------------------------
    def _design_matrix(self) -> np.ndarray:
        """x_evals as one contiguous n x d array; rows already copied stay (the list only grows during a run), which
        avoids re-stacking several hundred small arrays every iteration."""
        n = len(self.x_evals)
        buf = self.__X_buf
        if buf is None or buf.shape[0] < n or self.__X_rows > n:
            buf = np.empty((max(n, self.budget), self.dimension), dtype=np.float64)
            self.__X_buf, self.__X_rows = buf, 0
        for i in range(self.__X_rows, n):
            buf[i] = self.x_evals[i]
        self.__X_rows = n
        return buf[:n]

    def _take_noise(self, shape) -> np.ndarray:
        if not self.__noise_pending:
            return np.random.normal(0, 1e-8, size=shape)
        nz = self.__noise_res.get()
        self.__noise_pending = False
        if isinstance(nz, BaseException):
            raise nz
        if nz.shape != tuple(shape):
            raise RuntimeError("noise prefetch out of step with the run (a draw of another shape left the RNG)")
        return nz

    def _noise_worker(self, req, res) -> None:
        while True:
            shape = req.get()
            if shape is None:
                return
            try:
                res.put(np.random.normal(0, 1e-8, size=shape))   # numpy releases the GIL while it generates
            except BaseException as e:  # noqa: BLE001 - handed to the thread that asked
                res.put(e)

    def _prefetch_noise(self) -> None:
        """Called once the current iteration's noise is consumed: the next iteration (if there is one) has as many more
        points as this one proposes (one, or q).  One worker thread per run (creating a thread per iteration cost 0.24 ms of
        every iteration)."""
        n, q_eff = len(self.x_evals), self._q_eff()
        if not self.__prefetch_on or self.__noise_pending or n + q_eff >= self.budget:
            return
        if self.__noise_thread is None:
            import queue
            import threading
            self.__noise_req, self.__noise_res = queue.SimpleQueue(), queue.SimpleQueue()
            self.__noise_thread = threading.Thread(target=self._noise_worker, args=(self.__noise_req, self.__noise_res),
                                                   daemon=True)
            self.__noise_thread.start()
        self.__noise_pending = True
        self.__noise_req.put((n + q_eff, self.dimension))

    def _stop_noise_worker(self) -> None:
        if self.__noise_thread is None:
            return
        self.__noise_req.put(None)
        self.__noise_thread.join()
        self.__noise_thread, self.__noise_pending = None, False
        self.__noise_req = self.__noise_res = None

    def _transform_points_to_reduced_space(self) -> None:
        if len(self.x_evals) < 2:
            if len(self.x_evals) == 1:
                self.__z_evals = [np.zeros(1)]
            return
        X = self._design_matrix()
        ranks = self._calculate_ranks()
        noise = self._take_noise(X.shape)                      # same draw, same global RNG as the reference
        start = perf_counter()
        if self.__fused and not self._fit_gp:
            # rows A-H in one enqueue: the GP conditioning is queued right behind the projection and runs while the
            # wPCA results travel back (`_initialize_model` then has nothing left to launch)
            self._ctx.wpca_gp_condition(
                X, np.array(self.f_evals, dtype=np.float64), ranks=ranks, maximize=self.maximization,
                var_threshold=self.var_threshold, n_components=self.n_components, noise=noise,
                lengthscale=LENGTHSCALE, gp_noise=NOISE, kernel=_native.KERNEL_MATERN52, collect=False)
            self.__gp_pending = True
            # While the device runs the eigen-decomposition the host builds the scrambled Sobol engine of this
            # iteration's initial-condition draw (0.15 ms) - with LAST iteration's k, which is this iteration's k
            # almost always.  Same draws from torch's global generator at the same place of its stream (nothing else
            # consumes it between here and the optimiser); if k did change the generator is put back and the engine
            # is built later, as without the guess.
            self.__engine_ready, guess, saved = None, None, None
            k_prev = self.reduced_space_dim_num
            if self.__speculate_engine and k_prev:
                import torch
                saved = torch.get_rng_state()
                guess = _init.scrambled_sobol_engine(int(k_prev))
            res = self._ctx.wpca_results()
            if guess is not None:
                if res["k"] == k_prev:
                    self.__engine_ready = guess
                else:
                    torch.set_rng_state(saved)
        else:
            res = self._ctx.wpca(X, ranks=ranks, maximize=self.maximization, var_threshold=self.var_threshold,
                                  n_components=self.n_components, noise=noise, want_Z=False, want_full=True)
        self.timing_logs["pca"].append(perf_counter() - start)
        self.data_mean = res["data_mean"]
        self.component_matrix = res["components"]
        self.explained_variance_ratio = res["evr"]
        self.reduced_space_dim_num = res["k"]
        self.pca = _FittedPCA(res["components"], res["pca_mean"], res["evr"], res["k"])
        if self.verbose:
            k = res["k"]
            print(f"Using {k} principal components with {np.sum(res['evr'][:k]) * 100:.2f}% explained variance")
        # the reduced coordinates stay on the device (the reference keeps them in `__z_evals` only to
        # rebuild bounds and the GP input, both of which happen on the device here)
        self.__z_evals = [res["k"]] * X.shape[0]

    # ---- rows D-H ---------------------------------------------------------------------------------
    def _initialize_model(self, **kwargs):
        if not self.__z_evals:
            return
        start = perf_counter()
        if self.__gp_pending:              # already enqueued together with the wPCA
            self.timing_logs["SingleTaskGP"].append(perf_counter() - start)
            return
        if self._fit_gp:                  # the fit leaves the context conditioned at the fitted hyperparameters
            self.gp_hyperparameters = fit_gp_hyperparameters(self._ctx, np.array(self.f_evals, dtype=np.float64), ard=self._ard)
            self.timing_logs["SingleTaskGP"].append(perf_counter() - start)
            return
        # enqueue only: the device conditions the GP while the host prepares the Sobol engine (gp_wait below)
        self._ctx.gp_condition(np.array(self.f_evals, dtype=np.float64), lengthscale=LENGTHSCALE, noise=NOISE,
                                kernel=_native.KERNEL_MATERN52, wait=False)
        self.__gp_pending = True
        self.timing_logs["SingleTaskGP"].append(perf_counter() - start)

    # ---- rows J-N ---------------------------------------------------------------------------------
    def optimize_acqf_and_get_observation(self) -> np.ndarray:
        ctx, cfg = self._ctx, self._torch_config
        acq = self.acquisition_function
        num_restarts, raw_samples, batch_limit = cfg["NUM_RESTARTS"], cfg["RAW_SAMPLES"], 5
        start = perf_counter()
        # Like the reference, where gpytorch's Gram/Cholesky happen lazily inside optimize_acqf, the wait for the
        # conditioning is accounted here; the scrambled Sobol engine (needs only k) is built meanwhile.
        engine, self.__engine_ready = self.__engine_ready, None
        if engine is None:
            engine = _init.scrambled_sobol_engine(ctx.k)
        bounds = ctx.acq_bounds()          # needs only the statistics kernel, not the factorisation
        t0 = perf_counter()
        raw = _init.draw_sobol(bounds, raw_samples, engine)
        self.phase_breakdown["sobol"] = self.phase_breakdown.get("sobol", 0.0) + perf_counter() - t0
        raw_vals = None
        one_call = self._scores_in_one_call(acq)
        if self.__gp_pending and self.__early_scoring and one_call:
            self.__gp_pending = False      # the optimiser's one call waits for the conditioning, scores and picks
        elif self.__gp_pending and self.__early_scoring:
            # the raw samples are scored right behind the conditioning on the stream: one wait for both
            t0 = perf_counter()
            raw_vals = ctx.gp_wait_eval(raw, acq.device_scalar, acq.maximize, acq.acq_code)
            self.__gp_pending = False
            self.phase_breakdown["raw_eval"] = self.phase_breakdown.get("raw_eval", 0.0) + perf_counter() - t0
        elif self.__gp_pending:
            ctx.gp_wait()
            self.__gp_pending = False
        new_z, infos = _acqopt.propose(
            ctx, bounds, acq.device_scalar, acq.maximize, acq.acq_code, num_restarts, raw_samples, batch_limit, 200,
            q_eff=self._q_eff(), strategy=self._q_strategy, f_evals=self.f_evals,
            raw=raw, raw_vals=raw_vals, breakdown=self.phase_breakdown,
            trace=self.trace[-1] if self._record_trace else None, one_call=one_call,
            before_lbfgsb=self._prefetch_noise)   # the draw overlaps with the time inside the library.  With the one call it
        # starts just before that call: scoring, pick and optimiser are native and hold no torch op it could crowd.  With the
        # three calls it starts after the initial pick: any earlier it shares the core with the pick's torch ops and doubles
        # their time (0.10 -> 0.21 ms)
        self.timing_logs["optimize_acqf"].append(perf_counter() - start)
        self.lbfgsb_info.extend(infos)
        return new_z

    # ---- row O ------------------------------------------------------------------------------------
    def _transform_point_to_original_space(self, z: np.ndarray) -> np.ndarray:
        if self.pca is None:
            return np.random.uniform(self.bounds[:, 0], self.bounds[:, 1])
        return self._ctx.inverse_map(z)

    def reset(self):
        super().reset()
        self.__z_evals = []
        self.pca = None
        self.explained_variance_ratio = None
