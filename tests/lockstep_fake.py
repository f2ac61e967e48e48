"""A scripted stand-in for `pcabo._native.Batch`, and the cases that pin the lock-step iteration of pcabo/batchrun.py with it.

`FakeBatch` is pure numpy: it answers every call `BatchedPCABO` / `BatchedVanillaBO` make on a batch with cheap deterministic
numbers, writes every call with a short hash of every array argument into a call log, and a script table
`(event, run, n) -> value` forces the rare paths of the loop (EVENTS).  Everything else in a case is real: the runs' numpy and
`HostMT` generators, `_native.sobol_draw_rows`, `pcabo.initializers`, `lhs_center`, `BBOBProblem`, the pool threads.  So a case
pins which calls the loop makes, in which order, with which bits, which draws it takes from which generator, where it yields,
what it records and what it warns about - on a machine without a GPU.

tests/test_batchrun_lockstep_cpu.py holds every case to tests/golden/batch_lockstep_digests.json, which was recorded with
pcabo/batchrun.py as it stood at commit RECORDED_FROM.  To record it again put that commit's batchrun.py back and run

    python tests/lockstep_fake.py > tests/golden/batch_lockstep_digests.json
"""
import hashlib
import itertools
import json
import os
import sys
import warnings

import numpy as np

RECORDED_FROM = "0a293b4"          # the commit whose pcabo/batchrun.py produced tests/golden/batch_lockstep_digests.json
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_lockstep_digests.json")

FID, B, DIM, BUDGET, N_DOE = 15, 4, 6, 26, 10
EVENTS = ("failed", "opt_status", "score_status", "score_nan", "oob", "fit_status", "fit_warnflag")
# (event, run, n) -> value.  Parking events take a run out for good, so no one script can hold all of them with four runs: the
# acquisition of a case chooses its script, the fit events join when the case fits.
SCRIPTS = {
    "EI": {("failed", 0, 12): True, ("oob", 2, 13): True, ("opt_status", 2, 16): -4, ("score_status", 3, 18): 3,
           ("failed", 0, 20): True},
    "PI": {("failed", 1, 11): True, ("opt_status", 0, 14): -7, ("score_nan", 2, 16): True, ("oob", 3, 17): True,
           ("failed", 3, 22): True},
    "UCB": {("failed", 3, 11): True, ("opt_status", 2, 13): -7, ("score_nan", 0, 17): True, ("oob", 1, 18): True,
            ("opt_status", 3, 21): -4, ("failed", 1, 16): True},
}
FIT_SCRIPT = {("fit_warnflag", 3, 12): 1, ("fit_warnflag", 1, 14): 2, ("fit_status", 1, 19): 2}
ACQUISITIONS = {"EI": dict(acquisition_function="expected_improvement"),
                "PI": dict(acquisition_function="probability_of_improvement"),
                "UCB": dict(acquisition_function="upper_confidence_bound", ucb_beta=2)}
TRACE = {"off": dict(record_trace=False), "on": dict(record_trace=True),
         "filter": dict(record_trace=True, trace_filter=lambda b, n: (b + n) % 3 == 0)}
FULL_LOGS = ("pca-group-EI-fit-off", "pca-device-EI-fit-off", "vanilla-group-EI-fit-off", "vanilla-device-EI-fit-off")    # kept call by call


def cases():
    """case id -> (class name, constructor keywords, script)."""
    out = {}
    for cls, kern, acq, fit, tr in itertools.product(("pca", "vanilla"), ("group", "device"), ACQUISITIONS, (False, True), TRACE):
        script = {**SCRIPTS[acq], **(FIT_SCRIPT if fit else {})}
        out["%s-%s-%s-%s-%s" % (cls, kern, acq, "fit" if fit else "nofit", tr)] = (
            cls, dict(acq_kernel=kern, fit_gp=fit, **ACQUISITIONS[acq], **TRACE[tr]), script)
    for cls in ("pca", "vanilla"):
        out["%s-group-EI-nofit-on-max" % cls] = (cls, dict(acq_kernel="group", maximization=True, record_trace=True), dict(SCRIPTS["EI"]))
    return out


def _h(a) -> str:
    if a is None:
        return "none"
    a = np.asarray(a)
    m = hashlib.blake2b(digest_size=5)
    m.update(("%s%s" % (a.dtype.str, a.shape)).encode())
    m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def _value(x):
    return -np.mean((np.asarray(x, dtype=np.float64) - 0.25) ** 2, axis=-1)


class _FakeContext:
    """Run b's context inside the fake batch (`Batch.ctx[b]`): the calls of botorch's retry, and the best_f dtype switch."""

    def __init__(self, batch, b):
        self.batch, self.b = batch, b

    def match_best_f_dtype(self, best_f):
        f64 = isinstance(best_f, np.floating) and best_f.dtype == np.float64
        self.batch._log("ctx%d.match_best_f_dtype" % self.b, "f64" if f64 else "f32")

    def acq_eval(self, Xq, best_f, maximize=False, acq=0, grad=True):
        assert not grad
        self.batch._log("ctx%d.acq_eval" % self.b, _h(Xq), repr(float(best_f)), int(bool(maximize)), int(acq))
        return self.batch._values(Xq, acq)

    def optimize_acqf(self, ics, bounds, best_f, maximize=False, acq=0, batch_limit=5, maxiter=200):
        bt = self.batch
        bt._log("ctx%d.optimize_acqf" % self.b, _h(ics), _h(bounds), repr(float(best_f)), int(bool(maximize)), int(acq),
                int(batch_limit), int(maxiter))
        cand, vals, info = bt._optimise_one(self.b, ics, bounds, acq, batch_limit, retry=True)
        return cand, vals, info, False


class FakeBatch:
    """The surface of `pcabo._native.Batch` that pcabo/batchrun.py uses.  `script`: see EVENTS; an entry is used up when it fires
    (`fired`).  `log`: one line per call.  `busy()` is not logged: how often a driver polls it is the driver's business."""
    script = {}                     # set by run_case before the runner builds its batch
    created = []                    # every instance, in order (a runner drops its batch in finish())

    def __init__(self, B, max_n, max_d, max_q=512, device=0, workers=0, group_acq=True, device_lbfgsb=0):
        self.B, self.max_n, self.max_d, self.max_q, self.device = B, max_n, max_d, max_q, device
        self.device_lbfgsb = int(device_lbfgsb)
        self.n = self.d = 0
        self.k = np.zeros(B, dtype=np.int32)
        self.fit_rounds = 0
        self.active = [True] * B
        self.ctx = [_FakeContext(self, b) for b in range(B)]
        self.log, self.fired, self.script = [], [], dict(type(self).script)
        self._last_k, self._vanilla, self._raw_buf = None, False, None
        # (the trailing 0 stood for an option of Batch that has been removed; the recorded digests of the logs include it)
        self._log("Batch", B, max_n, max_d, max_q, device, workers, int(bool(group_acq)), self.device_lbfgsb, 0)
        type(self).created.append(self)

    def _log(self, name, *args):
        self.log.append(" ".join([name] + [str(a) for a in args]))

    def _event(self, event, b):
        v = self.script.pop((event, b, self.n), None)
        if v is not None:
            self.fired.append((event, b, self.n))
        return v

    # ---- conditioning ------------------------------------------------------------------------------------------------
    def wpca_gp_condition_begin(self, X, ranks, noise, y, maximize=False, var_threshold=0.95, n_components=0,
                                lengthscale=0.6931471805599453, gp_noise=0.006737946999085467, kernel=0):
        _, self.n, self.d = np.asarray(X).shape
        self._vanilla = False
        self._log("wpca_gp_condition_begin", _h(X), _h(ranks), _h(noise), _h(y), int(bool(maximize)), var_threshold,
                  n_components, lengthscale, gp_noise, kernel)

    def gp_condition_begin(self, Z, y, norm_bounds=None, lengthscale=0.6931471805599453, gp_noise=0.006737946999085467, kernel=0):
        _, self.n, self.d = np.asarray(Z).shape
        self._vanilla = True
        self.k = np.full(self.B, self.d, dtype=np.int32)
        self._log("gp_condition_begin", _h(Z), _h(y), _h(norm_bounds), lengthscale, gp_noise, kernel)

    def wpca_results(self):
        # a run's k moves every third iteration, at another iteration for every run: the engine built with last k is wrong there
        k = np.array([2 + ((self.n + b) // 3) % 3 for b in range(self.B)], dtype=np.int32)
        if self._last_k is not None:
            for b in range(self.B):
                if self.active[b] and k[b] != self._last_k[b]:
                    self.fired.append(("k_changed", b, self.n))
        self.k = self._last_k = k
        self._log("wpca_results", _h(k))
        return [{"data_mean": None, "pca_mean": None, "components": None, "evr": None, "k": int(k[b]), "Z": None}
                for b in range(self.B)]

    def acq_bounds(self):
        buf = self.acq_bounds_packed = np.zeros((self.B, 2 * self.max_d))
        for b in range(self.B):
            k = int(self.k[b])
            buf[b, :k] = -(1.0 + 0.1 * b)
            buf[b, k: 2 * k] = 1.0 + 0.02 * (self.n % 7)
        self._log("acq_bounds")
        return [buf[b, : 2 * int(self.k[b])].reshape(2, int(self.k[b])).copy() for b in range(self.B)]

    def gp_fit(self, theta0=None):
        self._log("gp_fit", theta0)
        self.fit_rounds = 5 + self.n % 3
        out = []
        for b in range(self.B):
            if not self.active[b]:
                out.append({"status": 1})
                continue
            status = self._event("fit_status", b)
            if status:
                out.append({"status": int(status)})
                continue
            flag = self._event("fit_warnflag", b) or 0
            out.append({"noise": 0.01 + 1e-3 * b, "mean": 0.5 * self.n, "lengthscale": 0.7, "loss": 1.0 + b, "iterations": 4 + b,
                        "evaluations": 6 + (self.n + b) % 4, "warnflag": int(flag), "task": 3 if flag else 1, "status": 0})
        return out

    # ---- scoring -----------------------------------------------------------------------------------------------------
    def raw_row_buffer(self, q):
        if self._raw_buf is None or self._raw_buf.shape != (self.B, q * self.max_d):
            self._raw_buf = np.zeros((self.B, q * self.max_d))
        self._log("raw_row_buffer", q)
        return self._raw_buf

    @staticmethod
    def _values(X, acq):
        v = _value(X)
        return np.exp(v) if acq == 1 else v          # (probability of improvement: non-negative values)

    def gp_eval_begin(self, Xq_list, best_f, maximize=False, acq=0):
        self._log("gp_eval_begin", " ".join(_h(x) for x in Xq_list), _h(np.asarray(best_f, dtype=np.float64)), int(bool(maximize)),
                  int(acq), "in_row_buffer=%d" % all(x.base is self._raw_buf for x in Xq_list))
        return ([np.array(x, dtype=np.float64) for x in Xq_list], int(acq))

    def gp_eval_end(self, token):
        raw, acq = token
        vals = np.stack([self._values(x, acq) for x in raw])
        status = np.zeros(self.B, dtype=np.int32)
        for b in range(self.B):
            if self.active[b]:
                status[b] = self._event("score_status", b) or 0
                if self._event("score_nan", b):
                    vals[b, 3] = np.nan
        self._log("gp_eval_end", _h(vals), _h(status))
        return vals, status

    # ---- optimisation ------------------------------------------------------------------------------------------------
    def _optimise_one(self, b, ics, bounds, acq, batch_limit, retry=False):
        ics, bounds = np.asarray(ics, dtype=np.float64), np.asarray(bounds, dtype=np.float64)
        nr = ics.shape[0]
        ng = (nr + batch_limit - 1) // batch_limit
        cand = np.clip(0.9 * ics + 0.01, bounds[0], bounds[1])
        if not retry and self._event("oob", b):
            cand = cand * 0.0 + bounds[1] + 3.0       # every candidate outside the box it was to stay in
        vals = self._values(cand, acq)
        info = np.array([[3 + (b + self.n + g) % 5, 4 + (b + self.n + g) % 7 + int(retry), 0, 1] for g in range(ng)], dtype=np.int32)
        return cand, vals, info

    def _optimise(self, ics_list, bounds_list, acq, batch_limit):
        outs, status = [], np.zeros(self.B, dtype=np.int32)
        for b in range(self.B):
            k, nr = int(self.k[b]), ics_list[0].shape[0]
            if not self.active[b]:
                ng = (nr + batch_limit - 1) // batch_limit
                outs.append((np.zeros((nr, k)), np.zeros(nr), np.zeros((ng, 4), dtype=np.int32), False))
                continue
            cand, vals, info = self._optimise_one(b, ics_list[b], bounds_list[b], acq, batch_limit)
            status[b] = self._event("opt_status", b) or 0
            outs.append((cand, vals, info, bool(self._event("failed", b))))
        return outs, status

    def _log_optimise(self, name, ics_list, bounds_list, best_f, maximize, acq, batch_limit, maxiter):
        self._log(name, " ".join(_h(x) for x in ics_list), " ".join(_h(x) for x in bounds_list),
                  _h(np.asarray(best_f, dtype=np.float64)), int(bool(maximize)), int(acq), int(batch_limit), int(maxiter))

    def optimize_begin(self, ics_list, bounds_list, best_f, maximize=False, acq=0, batch_limit=5, maxiter=200):
        self._log_optimise("optimize_begin", ics_list, bounds_list, best_f, maximize, acq, batch_limit, maxiter)
        return ([np.array(x) for x in ics_list], [np.array(x) for x in bounds_list], int(acq), int(batch_limit))

    def optimize_end(self, token):
        self._log("optimize_end")
        return self._optimise(*token)

    def optimize_acqf(self, ics_list, bounds_list, best_f, maximize=False, acq=0, batch_limit=5, maxiter=200):
        self._log_optimise("optimize_acqf", ics_list, bounds_list, best_f, maximize, acq, batch_limit, maxiter)
        return self._optimise(ics_list, bounds_list, int(acq), int(batch_limit))

    # ---- inverse map -------------------------------------------------------------------------------------------------
    def inverse_map_begin(self, z_list):
        self._log("inverse_map_begin", " ".join(_h(z) for z in z_list))
        self._z = [np.asarray(z, dtype=np.float64).ravel() for z in z_list]

    def inverse_map_end(self):
        self._log("inverse_map_end")
        j = np.arange(self.d)
        return np.stack([3.0 * z[j % z.size] + 0.1 * j for z in self._z])

    # ---- the rest ----------------------------------------------------------------------------------------------------
    def set_active(self, active):
        self.active = [bool(a) for a in active]
        self._log("set_active", "".join("1" if a else "0" for a in self.active))

    def busy(self):
        return False

    def close(self):
        self._log("close")


# ---- a case: one whole batch under the fake, and what is kept of it ------------------------------------------------------
def _canon(m, x):
    """Feed `x` (arrays, tensors, scalars and containers of them) into the hash `m` with types and shapes."""
    if isinstance(x, dict):
        for key in sorted(x):
            m.update(("{%s:" % key).encode())
            _canon(m, x[key])
    elif isinstance(x, (list, tuple)):
        m.update(("[%d:" % len(x)).encode())
        for v in x:
            _canon(m, v)
    elif hasattr(x, "numpy") and not isinstance(x, np.generic):           # a torch tensor
        _canon(m, x.numpy())
    elif isinstance(x, (np.ndarray, np.generic)):
        a = np.asarray(x)
        m.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        m.update(np.ascontiguousarray(a).tobytes())
    elif isinstance(x, float):
        m.update(("f" + x.hex()).encode())
    else:
        m.update(("%s=%r" % (type(x).__name__, x)).encode())


def _d(x) -> str:
    m = hashlib.blake2b(digest_size=6)
    _canon(m, x)
    return m.hexdigest()


def run_case(case, drive: str):
    """One case (an entry of cases()) driven by `iteration()` ("iteration") or through `run_interleaved([r])` ("interleaved"),
    with `_native.Batch` already replaced by FakeBatch.  Returns (digests by field, call log)."""
    from pcabo import batchrun
    from pcabo.bbob import BBOBProblem
    cls, kw, script = case
    FakeBatch.script, FakeBatch.created = script, []
    r = (batchrun.BatchedPCABO if cls == "pca" else batchrun.BatchedVanillaBO)(
        [BBOBProblem(FID, i, DIM) for i in range(B)], [1000 * FID + 10 * DIM + i for i in range(B)], BUDGET, N_DOE, **kw)
    labels, steps = [], r._iteration_steps

    def recorded_steps():
        for label in steps():
            labels.append(label)
            yield label
        labels.append("end")
    r._iteration_steps = recorded_steps
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if drive == "iteration":
            r.run()
        else:
            batchrun.run_interleaved([r])
    rs, tg = r._rs, r._tg
    (bt,) = FakeBatch.created
    assert all(f is not None or len(r.f_evals[b]) == BUDGET for b, f in enumerate(r.failed))
    out = {
        "x_evals": _d(r.x_evals), "f_evals": _d(r.f_evals), "best": _d([r.current_best, r.current_best_index]),
        "failed": _d(r.failed), "retries": _d(r.retries), "k_hist": _d(r.k_hist), "lbfgsb_info": _d(r.lbfgsb_info),
        "trace": _d(r.trace), "trace_entries": len(r.trace),
        "fit": _d([r.fit_rounds, r.fit_evaluations, [hp is not None for hp in r.gp_hyperparameters]]),
        "numpy_generators": _d([g.get_state() for g in rs]), "torch_generators": _d([g.get_state() for g in tg]),
        "warnings": _d(sorted((w.category.__name__, str(w.message)) for w in caught)), "warnings_raised": len(caught),
        "timing_keys": ",".join(sorted(r.timing)), "labels": _d(labels), "fired": sorted("%s/%d/%d" % e for e in bt.fired),
        "calls": len(bt.log), "call_log": _d(bt.log),
    }
    return out, bt.log


def record() -> str:
    """The content of tests/golden/batch_lockstep_digests.json from the pcabo/batchrun.py that is in the tree."""
    from pcabo import _native
    real = _native.Batch
    _native.Batch = FakeBatch
    try:
        out = {"recorded_from": RECORDED_FROM,
               "shape": {"function": FID, "runs": B, "dimension": DIM, "budget": BUDGET, "n_DoE": N_DOE}, "cases": {}, "call_logs": {}}
        for cid, case in cases().items():
            got, log = run_case(case, "iteration")
            again, _ = run_case(case, "interleaved")
            if got != again:
                raise SystemExit("%s: iteration() and run_interleaved disagree: %r / %r" % (cid, got, again))
            out["cases"][cid] = got
            if cid in FULL_LOGS:
                out["call_logs"][cid] = log
    finally:
        _native.Batch = real
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "para-ortho-pca-bo_amd"), root]
    sys.stdout.write(record())
