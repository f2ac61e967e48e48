"""sha256 of what short whole runs of the single-run optimisers leave behind - Algorithms.PCA_BO and Algorithms.Vanilla_BO through
their public surface only, so the same file runs on any commit that has the keywords: the bytes of x_evals, f_evals, the flattened
lbfgsb_info, the per-iteration reduced_space_dim_num (PCA_BO) and the last iteration's gp_hyperparameters (fit cases).
  BBOB f15 instance 1 (pcabo.bbob.BBOBProblem), random_seed 7, n_DoE 12, budget 22: ten iterations; d = 10 for PCA_BO (k < d, and k
  can change between iterations), d = 5 for Vanilla_BO
  pca_* / vanilla_*   one case per keyword that selects another path (CASES below); `smoke` is constructed with SMOKE_TEST=1 in the
                      environment (set around the constructor only); `trace` also hashes every trace entry's n and best_f
  *_visit             fantasy_points=2, stepped with _start / _bo_iteration / _finish; after iteration 4: posterior of 3 points with
                      the covariance, posterior_samples(seed=3, n_samples=2), loo() and a believer fantasy of 2 points with loo()
                      inside - those outputs are hashed beside the trajectory
  pca_oob_seed{s}     the first of seeds 1..8 whose default PCA_BO run meets the out-of-bounds penalty (+-1000 in f_evals), if any
tests/golden/single_run_hashes.json holds the bits of the two classes before their shared part was written once.
    python tools/gpu_run_hashes.py            # print
    python tools/gpu_run_hashes.py --write    # regenerate (only after an INTENDED change of a run's arithmetic or RNG order)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "para-ortho-pca-bo_amd"):
    if os.path.join(ROOT, p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "single_run_hashes.json")
FID, INSTANCE, SEED, N_DOE, BUDGET = 15, 1, 7, 12, 22
DIM = {"pca": 10, "vanilla": 5}
VISIT_AFTER = 4                                              # iterations in front of the visit case's model queries
OOB_SEEDS = range(1, 9)
CASES = {
    "pca": {"default": {}, "group": {"acq_kernel": "group"}, "not_resident": {"resident": False},
            "unfused": {"fused_enqueue": False}, "late_scoring": {"early_scoring": False}, "no_engine_guess": {"engine_guess": False},
            "no_prefetch": {"prefetch_noise": False}, "trace": {"record_trace": True}, "fit": {"fit_gp": True},
            "fit_ard": {"fit_gp": True, "ard": True}, "pi": {"acquisition_function": "PI"},
            "ucb": {"acquisition_function": "UCB", "ucb_beta": 2.0}, "components3": {"n_components": 3}, "smoke": {}},
    "vanilla": {"default": {}, "not_resident": {"resident": False}, "fit": {"fit_gp": True}, "fit_ard": {"fit_gp": True, "ard": True},
                "pi": {"acquisition_function": "PI"}, "ucb": {"acquisition_function": "UCB", "ucb_beta": 2.0},
                "trace": {"record_trace": True}},
}


def case_names(cls: str) -> set:
    """Every case of a class that does not depend on what a run finds (the out-of-bounds case does)."""
    return {"%s_%s" % (cls, name) for name in CASES[cls]} | {cls + "_visit"}


def _h(a, dtype=np.float64) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def _h_dict(d: dict) -> dict:
    """Every entry of a result dict: numbers as the sha256 of their float64 bytes, anything else in the clear."""
    out = {}
    for key in sorted(d):
        v = np.asarray(d[key])
        out[key] = _h(v) if v.dtype.kind in "fiub" else str(d[key])
    return out


def _optimiser(cls: str, seed=SEED, smoke=False, **kwargs):
    from Algorithms import PCA_BO, Vanilla_BO
    saved = os.environ.get("SMOKE_TEST")
    if smoke:
        os.environ["SMOKE_TEST"] = "1"
    try:
        return {"pca": PCA_BO, "vanilla": Vanilla_BO}[cls](budget=BUDGET, n_DoE=N_DOE, random_seed=seed, **kwargs)
    finally:
        if smoke:
            if saved is None:
                del os.environ["SMOKE_TEST"]
            else:
                os.environ["SMOKE_TEST"] = saved


def _problem(cls: str):
    from pcabo.bbob import BBOBProblem
    return BBOBProblem(FID, INSTANCE, DIM[cls])


def _run(opt, problem, visit=None) -> list:
    """__call__ in its three pieces; returns reduced_space_dim_num after every iteration (None for Vanilla_BO).  `visit(opt)` is
    called once, after iteration VISIT_AFTER."""
    ks = []
    try:
        opt._start(problem)
        for it in range(opt.budget - opt.n_DoE):
            opt._bo_iteration(problem)
            ks.append(getattr(opt, "reduced_space_dim_num", None))
            if visit is not None and it + 1 == VISIT_AFTER:
                visit(opt)
    finally:
        opt._finish()
    return ks


def _record(opt, ks, fit=False, trace=False) -> dict:
    rec = {"x_evals": _h(np.vstack(opt.x_evals)), "f_evals": _h(opt.f_evals), "n": len(opt.f_evals),
           "lbfgsb_info": _h(np.concatenate([np.asarray(i).ravel() for i in opt.lbfgsb_info]), np.int64)}
    if ks[0] is not None:
        rec["k"] = [int(k) for k in ks]
    if fit:
        rec["gp_hyperparameters"] = _h_dict(opt.gp_hyperparameters)
    if trace:
        rec["trace_n"] = [int(t["n"]) for t in opt.trace]
        rec["trace_best_f"] = _h([t["best_f"] for t in opt.trace])
    return rec


def plain_case(cls: str, name: str) -> dict:
    kwargs = CASES[cls][name]
    opt = _optimiser(cls, smoke=name == "smoke", **kwargs)
    ks = _run(opt, _problem(cls))
    return _record(opt, ks, fit=bool(kwargs.get("fit_gp")), trace=bool(kwargs.get("record_trace")))


def visit_case(cls: str) -> dict:
    seen = {}
    points = np.random.default_rng(11).uniform(-4.0, 4.0, size=(5, DIM[cls]))

    def visit(opt):
        seen["posterior"] = _h_dict(opt.posterior(points[:3], covariance=True))
        seen["posterior_samples"] = _h_dict(opt.posterior_samples(points[:3], n_samples=2, seed=3))
        seen["loo"] = _h_dict(opt.loo())
        with opt.fantasy(points[3:]) as model:
            seen["fantasy_loo"] = _h_dict(model.loo())
    opt = _optimiser(cls, fantasy_points=2)
    ks = _run(opt, _problem(cls), visit)
    return {**_record(opt, ks), **seen}


def _default_pca_run(seed: int):
    opt = _optimiser("pca", seed=seed)
    return opt, _run(opt, _problem("pca"))


def first_oob_seed():
    """The first of OOB_SEEDS whose default PCA_BO run is penalised; None if none is."""
    for seed in OOB_SEEDS:
        opt, _ = _default_pca_run(seed)
        if np.any(np.abs(np.asarray(opt.f_evals)) == 1000):
            return seed
    return None


def class_cases(cls: str, oob_seed=None) -> dict:
    """All cases of one class; `oob_seed`: with PCA_BO's out-of-bounds case at that seed (None: without it)."""
    out = {"%s_%s" % (cls, name): plain_case(cls, name) for name in CASES[cls]}
    out[cls + "_visit"] = visit_case(cls)
    if oob_seed is not None:
        out["pca_oob_seed%d" % oob_seed] = _record(*_default_pca_run(oob_seed))
    return out


def compute() -> dict:
    return {**class_cases("pca", first_oob_seed()), **class_cases("vanilla")}


if __name__ == "__main__":
    res = compute()
    if "--write" in sys.argv:
        i = sys.argv.index("--write")
        out = sys.argv[i + 1] if len(sys.argv) > i + 1 else GOLDEN
        oob = [int(name[len("pca_oob_seed"):]) for name in res if name.startswith("pca_oob_seed")]
        with open(out, "w") as f:
            json.dump({"_comment": "tools/gpu_run_hashes.py --write on an MI355X, with the tree of commit abefd7a: before the "
                                   "single-run optimiser was written once for PCA_BO and Vanilla_BO",
                       "oob_seed": oob[0] if oob else None, "cases": res}, f, indent=1)
        print("written", out)
    else:
        print(json.dumps(res, indent=1))
