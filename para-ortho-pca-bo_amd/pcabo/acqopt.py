"""Host-side control flow of `botorch.optim.optimize_acqf(q=1, num_restarts, raw_samples, batch_limit=5, maxiter=200)`
as both optimisers of the reference call it (PCA_BO.py:607-614, Vanilla_BO.py:206-213), with every numerical step on
the device: raw-sample scoring (`Context.acq_eval`), multi-start L-BFGS-B (`Context.optimize_acqf`).  The RNG-consuming
steps (Sobol scramble bits, multinomial pick) run on torch's global CPU generator in botorch's order."""
from __future__ import annotations

import warnings
from time import perf_counter
from typing import Optional

import numpy as np

from . import _native
from . import initializers as _init


ALLOWED_ACQUISITION_FUNCTION_STRINGS = (
    "expected_improvement",
    "probability_of_improvement",
    "upper_confidence_bound",
)
ALLOWED_SHORTHAND_ACQUISITION_FUNCTION_STRINGS = {
    "EI": "expected_improvement",
    "PI": "probability_of_improvement",
    "UCB": "upper_confidence_bound",
}


def acquisition_long_name(name: str, odd_name: str = "Oddly defined name") -> str:
    """The long name of an acquisition given by its short or long name (reference PCA_BO.py:654-677): surrounding blanks dropped,
    a short name replaced by its long one, anything else ValueError(odd_name), where `{name}` stands for the stripped name.  Like
    the reference, a long name in another letter case passes as it is spelled - and then selects no acquisition class."""
    name = name.strip()
    if name in ALLOWED_SHORTHAND_ACQUISITION_FUNCTION_STRINGS:
        return ALLOWED_SHORTHAND_ACQUISITION_FUNCTION_STRINGS[name]
    if name.lower() in ALLOWED_ACQUISITION_FUNCTION_STRINGS:
        return name
    raise ValueError(odd_name.format(name=name))


def ucb_kappa(beta) -> float:
    """kappa = sqrt(beta) as botorch's UpperConfidenceBound forms it: it stores `torch.as_tensor(beta)` - float32 for a Python
    float - and takes `.sqrt()` of that tensor.  The device never takes the root: kappa travels in the `best_f` slot."""
    import torch
    return float(torch.as_tensor(float(beta)).sqrt())


def checked_ucb_beta(ucb_beta, acquisition_name: str) -> Optional[float]:
    """The `ucb_beta` keyword of the optimisers, validated where they are constructed: None stays None (UCB then fails as the
    reference's does); otherwise a finite float >= 0 together with the upper-confidence-bound acquisition, else ValueError."""
    if ucb_beta is None:
        return None
    beta = float(ucb_beta)
    if not (np.isfinite(beta) and beta >= 0.0):
        raise ValueError(f"ucb_beta must be finite and >= 0, got {ucb_beta!r}")
    if acquisition_name.strip().lower() not in ("ucb", "upper_confidence_bound"):
        raise ValueError(f"ucb_beta is the parameter of the upper-confidence-bound acquisition; it was given together with "
                         f"{acquisition_name!r}")
    return beta


def optimize_acqf(ctx: "_native.Context", bounds: np.ndarray, best_f: float, maximize: bool, acq_code: int,
                  num_restarts: int, raw_samples: int, batch_limit: int = 5, maxiter: int = 200, engine=None,
                  breakdown: Optional[dict] = None, trace: Optional[dict] = None, raw: Optional[np.ndarray] = None,
                  raw_vals: Optional[np.ndarray] = None, before_lbfgsb=None):
    """Returns (candidate[1, k], all restart candidates, their values, L-BFGS-B info).  `best_f`: the acquisition's scalar
    (the incumbent; for ACQ_UCB kappa - it takes the standardised Boltzmann pick like log-EI).  `engine`: a scrambled Sobol
    engine prepared earlier (same RNG consumption, earlier in time); `raw`: the raw samples already drawn from it
    (while the device was still factorising); `raw_vals`: their acquisition values if the caller already has them
    (`Context.gp_wait_eval`).  The retry path draws and scores afresh.  `before_lbfgsb()`: called once, after the
    initial conditions are picked (where PCA_BO starts the next iteration's noise draw on its worker thread)."""
    pb = breakdown if breakdown is not None else {}
    engines = [engine] if engine is not None and raw is None else []
    ready = [raw] if raw is not None else []
    ready_vals = [raw_vals] if raw is not None and raw_vals is not None else []

    def initial_conditions():
        t0 = perf_counter()
        raw = ready.pop() if ready else _init.draw_sobol(bounds, raw_samples, engines.pop() if engines else None)
        t1 = perf_counter()
        vals = ready_vals.pop() if ready_vals else ctx.acq_eval(raw, best_f, maximize, acq_code, grad=False)
        t2 = perf_counter()
        if acq_code == _native.ACQ_PI:
            idx = _init.initialize_q_batch_nonneg(vals, num_restarts)
        else:
            idx = _init.initialize_q_batch(vals, num_restarts)
        t3 = perf_counter()
        pb["sobol"] = pb.get("sobol", 0.0) + t1 - t0
        pb["raw_eval"] = pb.get("raw_eval", 0.0) + t2 - t1
        pb["init_pick"] = pb.get("init_pick", 0.0) + t3 - t2
        if trace is not None:
            trace.update(raw_vals=vals.copy(), ic_idx=np.asarray(idx).copy())
        return raw[idx]

    ics = initial_conditions()
    if before_lbfgsb is not None:
        before_lbfgsb()
    t_opt = perf_counter()
    cand, vals, info, failed = ctx.optimize_acqf(ics, bounds, best_f, maximize, acq_code, batch_limit=batch_limit,
                                                 maxiter=maxiter)
    pb["lbfgsb"] = pb.get("lbfgsb", 0.0) + perf_counter() - t_opt
    if failed:   # botorch: OptimizationWarning -> one retry with freshly drawn initial conditions
        warnings.warn("Optimization failed in `gen_candidates_scipy`; trying again with a new set of "
                      "initial conditions.", RuntimeWarning)
        if trace is not None:
            trace["retried"] = True
        ics = initial_conditions()
        cand, vals, info, failed = ctx.optimize_acqf(ics, bounds, best_f, maximize, acq_code,
                                                     batch_limit=batch_limit, maxiter=maxiter)
    best = int(np.argmax(vals))
    if trace is not None:
        trace.update(ics=ics.copy(), cands=cand.copy(), vals=vals.copy(), chosen=best, info=info.copy(),
                     k=int(cand.shape[1]))
    return cand[best].reshape(1, -1), cand, vals, info
