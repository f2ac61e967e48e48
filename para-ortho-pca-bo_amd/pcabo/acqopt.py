"""Host-side control flow of `botorch.optim.optimize_acqf(q=1, num_restarts, raw_samples, batch_limit=5, maxiter=200)`
as both optimisers of the reference call it (PCA_BO.py:607-614, Vanilla_BO.py:206-213), with every numerical step on
the device: raw-sample scoring (`Context.acq_eval`), multi-start L-BFGS-B (`Context.optimize_acqf`).  The RNG-consuming
steps (Sobol scramble bits, multinomial pick) run on torch's global CPU generator in botorch's order."""
from __future__ import annotations

import os
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


Q_STRATEGIES = ("kriging_believer", "constant_liar_min", "constant_liar_mean", "constant_liar_max")


def checked_q(q, q_strategy):
    """The `q` / `q_strategy` keywords of the optimisers, validated where they are constructed: q an integer >= 1 (a bool is not
    one), the strategy one of Q_STRATEGIES; ValueError otherwise.  Returns (int(q), q_strategy)."""
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or q < 1:
        raise ValueError(f"q must be an integer >= 1, got {q!r}")
    if q_strategy not in Q_STRATEGIES:
        raise ValueError(f"q_strategy must be one of {', '.join(Q_STRATEGIES)}; got {q_strategy!r}")
    return int(q), q_strategy


def liar_value(strategy: str, f_evals) -> float:
    """The value a constant-liar strategy gives every pending point: min / mean / max of the objective values seen so far."""
    f = np.asarray(f_evals, dtype=np.float64)
    return float({"constant_liar_min": f.min, "constant_liar_mean": f.mean, "constant_liar_max": f.max}[strategy]())


def moved_scalar(s, v, maximize: bool, acq_code: int):
    """The acquisition's scalar after a pending point took the value v: UCB's kappa stays, an incumbent moves to the better of
    the two (an unmoved best_f lets EI and PI propose the same point again: the variance there is gone, the mean is not)."""
    if acq_code == _native.ACQ_UCB:
        return s
    return max(s, v) if maximize else min(s, v)


ONE_CALL_ENV = "PCABO_ONE_CALL"      # "0": scoring, pick and optimiser of a single run stay three calls (A/B runs of one build)
ONE_CALL_WAKE_ENV = "PCABO_ONE_CALL_WAKE"      # "0": the one call leaves the stepping helper asleep until the optimiser needs it


def one_call_default() -> bool:
    return os.environ.get(ONE_CALL_ENV, "1") != "0"


def one_call_applies(ctx, acq_code: int, num_restarts: int, n_raw: int) -> bool:
    """Can the first attempt of `optimize_acqf` be `Context.propose_acqf`?  Not for PI (botorch's non-negative pick stays in
    torch), not with as many restarts as raw samples (no pick at all), not on a context that offers the three calls only (a
    stand-in for `_native.Context`), and not when the native generator is not this torch build's (`hostrng.native_ok`)."""
    if acq_code == _native.ACQ_PI or num_restarts >= n_raw or not callable(getattr(ctx, "propose_acqf", None)):
        return False
    from . import hostrng
    return hostrng.native_ok()


def optimize_acqf(ctx: "_native.Context", bounds: np.ndarray, best_f: float, maximize: bool, acq_code: int,
                  num_restarts: int, raw_samples: int, batch_limit: int = 5, maxiter: int = 200, engine=None,
                  breakdown: Optional[dict] = None, trace: Optional[dict] = None, raw: Optional[np.ndarray] = None,
                  raw_vals: Optional[np.ndarray] = None, before_lbfgsb=None, one_call: Optional[bool] = None):
    """Returns (candidate[1, k], all restart candidates, their values, L-BFGS-B info).  `best_f`: the acquisition's scalar
    (the incumbent; for ACQ_UCB kappa - it takes the standardised Boltzmann pick like log-EI).  `engine`: a scrambled Sobol
    engine prepared earlier (same RNG consumption, earlier in time); `raw`: the raw samples already drawn from it
    (while the device was still factorising); `raw_vals`: their acquisition values if the caller already has them
    (`Context.gp_wait_eval`).  The retry path draws and scores afresh.  `before_lbfgsb()`: called once, after the
    initial conditions are picked (where PCA_BO starts the next iteration's noise draw on its worker thread).
    `one_call` (None: `one_call_default()`): with `raw` given and `raw_vals` not, scoring, pick and optimiser are ONE native call
    (`Context.propose_acqf`, which also ends a conditioning in flight) on the state of torch's global generator - where
    `one_call_applies`.  `before_lbfgsb()` is then called just before that call.  Same results and the same generator state afterwards as the three calls."""
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

    def in_one_call():
        """The first attempt through Context.propose_acqf: (ics, cand, vals, info, failed), or None when the scores have no
        spread - nothing was drawn or optimised, and the scores wait in ready_vals for botorch's other paths."""
        import torch
        blob = torch.get_rng_state().numpy()
        if before_lbfgsb is not None:
            before_lbfgsb()
        r = ctx.propose_acqf(raw, blob, num_restarts, bounds, best_f, maximize, acq_code, batch_limit=batch_limit,
                             maxiter=maxiter, eta=_init.INIT_ETA, wake=os.environ.get(ONE_CALL_WAKE_ENV, "1") != "0")
        for key, t in zip(("raw_eval", "init_pick", "lbfgsb"), r["phase_seconds"]):
            pb[key] = pb.get(key, 0.0) + float(t)
        pb.setdefault("sobol", 0.0)
        if not r["picked"]:
            ready_vals.append(r["raw_vals"])
            return None
        ready.pop()
        torch.set_rng_state(torch.from_numpy(blob))
        if trace is not None:
            trace.update(raw_vals=r["raw_vals"].copy(), ic_idx=r["ic_idx"].copy())
        return r["ics"], r["cand"], r["vals"], r["info"], r["failed"]

    if one_call is None:
        one_call = one_call_default()
    first = None
    if one_call and raw is not None and raw_vals is None and one_call_applies(ctx, acq_code, num_restarts, len(raw)):
        first = in_one_call()
        before_lbfgsb = None               # (called already)
    if first is not None:
        ics, cand, vals, info, failed = first
    else:
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


def propose(ctx: "_native.Context", bounds: np.ndarray, best_f: float, maximize: bool, acq_code: int, num_restarts: int,
            raw_samples: int, batch_limit: int = 5, maxiter: int = 200, q_eff: int = 1, strategy: str = "kriging_believer",
            f_evals=None, breakdown: Optional[dict] = None, trace: Optional[dict] = None, raw: Optional[np.ndarray] = None,
            raw_vals: Optional[np.ndarray] = None, before_lbfgsb=None, one_call: Optional[bool] = None):
    """q_eff candidates of one iteration, one after the other on a model that takes every pending point in (DESIGN.md section
    18).  Proposal 0 is `optimize_acqf` with everything the caller prepared (`raw`, `raw_vals`, `before_lbfgsb`, `trace`); each
    later one is a whole `optimize_acqf` of its own - a fresh scrambled Sobol engine from torch's global generator, scoring by
    `Context.acq_eval`, pick, L-BFGS-B, botorch's retry - on the context extended by the point before it (`Context.gp_extend`)
    with the value v: the model's own mean there (kriging_believer) or min / mean / max of `f_evals` (constant_liar_*).  The
    scalar moves with v (`moved_scalar`).  `bounds` is held.  Whatever was appended is taken back before this returns or raises.
    A later proposal's trace is a dict of `optimize_acqf`'s keys plus `best_f` and `believed` in trace["proposals"].
    Returns (candidates[q_eff, k], [L-BFGS-B info per proposal])."""
    believer = strategy == "kriging_believer"
    if strategy not in Q_STRATEGIES:
        raise ValueError(f"q_strategy must be one of {', '.join(Q_STRATEGIES)}; got {strategy!r}")
    liar = None if believer or q_eff <= 1 else liar_value(strategy, f_evals)
    s, n0, cands, infos = best_f, None, [], []
    try:
        z, _, _, info = optimize_acqf(ctx, bounds, s, maximize, acq_code, num_restarts, raw_samples, batch_limit, maxiter,
                                      breakdown=breakdown, trace=trace, raw=raw, raw_vals=raw_vals, before_lbfgsb=before_lbfgsb,
                                      one_call=one_call)
        cands.append(z)
        infos.append(info)
        for _ in range(1, q_eff):
            v = float(ctx.gp_posterior(z)["mean"][0]) if believer else liar
            n = ctx.n
            ctx.gp_extend(z, None if believer else [v])
            n0 = n if n0 is None else n0
            s = moved_scalar(s, v, maximize, acq_code)
            tr = None
            if trace is not None:
                tr = {"best_f": s, "believed": v}
                trace.setdefault("proposals", []).append(tr)
            z, _, _, info = optimize_acqf(ctx, bounds, s, maximize, acq_code, num_restarts, raw_samples, batch_limit, maxiter,
                                          breakdown=breakdown, trace=tr)
            cands.append(z)
            infos.append(info)
    finally:
        if n0 is not None:
            ctx.gp_truncate(n0)
    return np.concatenate(cands, axis=0), infos
