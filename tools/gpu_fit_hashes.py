"""sha256 of what the GP fit's entry points return - loss, gradient and theta bytes - and the info quadruple (iterations, evaluations,
warnflag, task) in the clear, for the shared-lengthscale form (Context.gp_mll / gp_fit, Batch.gp_mll / gp_fit) and the per-input
form (Context.gp_mll_ard / gp_fit_ard), on the smallest states that reach each part of k_mll_grad / k_mll_finish and each rule of
FitRun:
  eval_n{n}_k{k}_t{i}   the nine shapes of tests/test_gpu_ard.py (one padded tile .. k = PCABO_MAXD) at its five thetas; `ard` at
                        theta i, `scalar` at (noise, mean constant) of theta i with rho = RHOS[i].  t4 is rho = 25 in both forms:
                        softplus's linear branch, derivative 1 in both (host_side.h; the shared form took the sigmoid there
                        until tests/test_gpu_mll_edges.py judged it, and its t4 gradients were regenerated with that fix)
  fit_n{n}_k{k}_{start} both fits at the three FIT_STATES of tests/ard_reference.py from the default and from a seeded start; from
                        the start `out` (one lengthscale outside the domain) the error code is recorded
  batch3                the first three states of tests/test_gpu_batch_fit.py (runs of different k), run 1 parked: Batch.gp_mll at
                        two sets of per-run thetas, Batch.gp_fit and fit_rounds
tests/golden/fit_hashes.json holds the bits of the library before the fit was written once for both forms (PCABO_LIB selects the
library).
    python tools/gpu_fit_hashes.py            # print
    python tools/gpu_fit_hashes.py --write    # regenerate (only after an INTENDED change of arithmetic)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "para-ortho-pca-bo_amd"):
    if os.path.join(ROOT, p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np
from ard_reference import FIT_STATES, ard_state, theta0
from test_gp_fit_cpu import THETA0
from test_gpu_ard import SHAPES, _state as eval_state, _thetas as ard_thetas
from test_gpu_batch_fit import D, N, _state as batch_state

GOLDEN = os.path.join(ROOT, "tests", "golden", "fit_hashes.json")
RHOS = (0.0, -0.5, 0.8, 15.0, 25.0)                          # the scalar form's rho beside theta i of the per-input form
INFO = ("iterations", "evaluations", "warnflag", "task")
B = 3                                                        # the batch: tests/test_gpu_batch_fit.py's first three states
BATCH_THETAS = [THETA0, (1e-4, 0.3, -0.5), (0.05, -0.2, 0.8), (0.3, 0.5, 25.0)]


def _h(a) -> str:
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert np.isfinite(a).all()
    return hashlib.sha256(a.tobytes()).hexdigest()


def _eval_record(r) -> dict:
    return {"loss": _h(r["loss"]), "grad": _h(r["grad"]), "theta": _h(r["theta"])}


def _fit_record(r) -> dict:
    return {"loss": _h(r["loss"]), "theta": _h(r["theta"]), "info": [int(r[key]) for key in INFO]}


def eval_cases(N_) -> dict:
    ctx = N_.Context(max_n=130, max_d=128, max_q=64)
    out = {}
    for n, k in SHAPES:
        Z, y = eval_state(n, k)
        for i, theta in enumerate(ard_thetas(n, k)):
            out["eval_n%d_k%d_t%d" % (n, k, i)] = {
                "rho": RHOS[i], "rho_max": float(theta[2:].max()),
                "scalar": _eval_record(ctx.gp_mll(y, (theta[0], theta[1], RHOS[i]), Z=Z)),
                "ard": _eval_record(ctx.gp_mll_ard(y, theta, Z=Z))}
    ctx.close()
    return out


def fit_starts(n, k) -> dict:
    """start -> (the scalar form's theta0, the per-input form's)"""
    rho = np.random.default_rng(2000 + n + k).uniform(-0.5, 0.5, size=k)
    out = np.zeros(k)
    out[k - 1] = -800.0                                      # softplus(-800) = 0
    return {"default": (theta0(1), theta0(k)), "seeded": (np.r_[0.02, 0.1, rho[0]], np.r_[0.02, 0.1, rho]),
            "out": (np.r_[0.01, 0.0, -800.0], np.r_[0.01, 0.0, out])}


def fit_cases(N_) -> dict:
    ctx = N_.Context(max_n=130, max_d=128, max_q=64)
    out = {}
    for seed, n, k in FIT_STATES:
        Z, y = ard_state(seed, n, k)
        for start, (th_s, th_a) in fit_starts(n, k).items():
            rec = {}
            for form, fit, th in (("scalar", ctx.gp_fit, th_s), ("ard", ctx.gp_fit_ard, th_a)):
                try:
                    rec[form] = _fit_record(fit(y, th, Z=Z))
                except N_.PcaboError as e:
                    rec[form] = {"status": int(e.code)}
            out["fit_n%d_k%d_%s" % (n, k, start)] = rec
    ctx.close()
    return out


def batch3_case(N_) -> dict:
    X, y, noise = (np.stack(a) for a in zip(*[batch_state(b) for b in range(B)]))
    ranks = np.argsort(np.argsort(y, axis=1), axis=1).astype(np.int64) + 1
    bt = N_.Batch(B, max_n=N, max_d=D, max_q=64)
    bt.wpca_gp_condition_begin(X, ranks, noise, y)
    out = {"k": [r["k"] for r in bt.wpca_results()]}
    bt.set_active([1, 0, 1])
    for shift in (0, 2):
        thetas = np.array([BATCH_THETAS[(b + shift) % len(BATCH_THETAS)] for b in range(B)])
        res = bt.gp_mll(thetas)
        assert res[1] == {"status": -1}
        for b in (0, 2):
            assert res[b]["status"] == 0
            out["mll%d_run%d" % (shift, b)] = _eval_record(res[b])
    fits = bt.gp_fit()
    assert fits[1] == {"status": -1}
    for b in (0, 2):
        assert fits[b]["status"] == 0
        out["fit_run%d" % b] = _fit_record(fits[b])
    out["fit_rounds"] = int(bt.fit_rounds)
    bt.close()
    return out


def compute() -> dict:
    from pcabo import _native as N_
    out = eval_cases(N_)
    out.update(fit_cases(N_))
    out["batch3"] = batch3_case(N_)
    return out


if __name__ == "__main__":
    res = compute()
    if "--write" in sys.argv:
        i = sys.argv.index("--write")
        out = sys.argv[i + 1] if len(sys.argv) > i + 1 else GOLDEN
        with open(out, "w") as f:
            json.dump({"_comment": "tools/gpu_fit_hashes.py --write on an MI355X, with the library of commit 6369d7c: before the "
                                   "fit was written once for shared and per-input lengthscales", "cases": res}, f, indent=1)
        print("written", out)
    else:
        print(json.dumps(res, indent=1))
