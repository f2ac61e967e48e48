"""sha256 of value + gradient from the single-run acquisition kernel k_acq_fast<SLAB,NB> in its two forms, on seeded GP states:
  plain     acq_eval (one launch per evaluation, in-launch combine) and optimize_acqf with PCABO_OPT_RESIDENT = 0;
  resident  optimize_acqf with the resident kernel (the default of a process alone on its GPU: every evaluation of the call
            goes through the mailbox to one launch).  The L-BFGS-B iterates follow every bit of every evaluation, so the
            hashed candidates, values and counters pin the resident kernel's value and gradient of each round.
The n cover every instantiation launch_acq uses (NP = 64 .. 384 with 16-row slabs, 448 and 512 with 32-row slabs), each with
k in {3, 17, 36, 40}.  tests/golden/acq_fast_hashes.json holds the bits of the kernel before its reductions were rewritten.
    python tools/gpu_acq_fast_hashes.py            # print
    python tools/gpu_acq_fast_hashes.py --write    # regenerate (only after an INTENDED change of arithmetic)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))
import numpy as np

NS = (60, 120, 180, 250, 300, 380, 420, 449)      # NP = 64 NB, NB = 1 .. 8
KS = (3, 17, 36, 40)
GOLDEN = os.path.join(ROOT, "tests", "golden", "acq_fast_hashes.json")


def _h(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def compute() -> dict:
    from pcabo import _native as N
    out = {}
    rng = np.random.default_rng(2025)
    for n in NS:
        for k in KS:
            Z = rng.uniform(0, 1, (n, k)); y = rng.normal(size=n)
            c = N.Context(max_n=max(n, 64), max_d=max(k, 2), max_q=64)
            c.gp_condition(y, Z=Z)
            best = float(y.min())
            rec = {}
            for q in (10, 3):
                Xq = rng.uniform(0.05, 0.95, (q, k))
                val, g = c.acq_eval(Xq, best, False, N.ACQ_LOG_EI, grad=True)
                assert np.isfinite(val).all() and np.isfinite(g).all()
                rec[f"plain_q{q}"] = {"val": _h(val), "grad": _h(g)}
            ics = rng.uniform(0.1, 0.9, (10, k))
            bounds = np.vstack([np.zeros(k), np.ones(k)])
            for mode, opt in (("resident", 1), ("plain", 0)):
                c.set_option(N.OPT_RESIDENT, opt)
                cand, vals, info, failed = c.optimize_acqf(ics, bounds, best, False, N.ACQ_LOG_EI, batch_limit=5, maxiter=60)
                rec[f"optimize_{mode}"] = {"cand": _h(cand), "vals": _h(vals), "info": _h(info)}
            c.set_option(N.OPT_RESIDENT, 1)
            out[f"{n},{k}"] = rec
            c.close()
    return out


if __name__ == "__main__":
    res = compute()
    if "--write" in sys.argv:
        i = sys.argv.index("--write")
        out = sys.argv[i + 1] if len(sys.argv) > i + 1 else GOLDEN
        with open(out, "w") as f:
            json.dump({"_comment": "tools/gpu_acq_fast_hashes.py --write on an MI355X (k_acq_fast with one wave_sum per value, "
                                   "before the multi-value reductions)", "cases": res}, f, indent=1)
        print("written", out)
    else:
        print(json.dumps(res, indent=1))
