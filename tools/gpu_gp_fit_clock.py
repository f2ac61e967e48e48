"""Cost of the opt-in GP hyperparameter fit (Context.gp_fit) on the GPU: one fit per shape, device-synchronised host clocks
(every call below returns after a wait on the stream), after a warm-up of each call at each shape.

Prints per shape: evaluations per fit, ms per fit, ms per evaluation (fit time / evaluations), ms of one evaluation alone
(gp_mll), ms of the conditioning alone at the same hyperparameters (gp_condition), and the marginal-likelihood share of an
evaluation, (gp_mll - gp_condition) / gp_mll: k_mll_grad + k_mll_finish + the 48-byte copy.  Kernel times come from a separate
run under `rocprofv3 --kernel-trace --stats` (one shape per run: --shapes 1050x89).

--ard adds the fit with one lengthscale per input (Context.gp_fit_ard / gp_mll_ard: the ARD form of k_mll_grad + k_mll_finish and a copy of
5 + KP doubles) on the same state, next to the scalar fit: evaluations, ms per fit, ms per evaluation, ms of gp_mll_ard alone and the
two losses.  --relevant R lets y depend on the first R inputs only (0: on all of them, the scalar tool's state), the setting ARD is for.

usage: gpu_gp_fit_clock.py [--shapes 450x36,1050x89] [--reps 5] [--ard] [--relevant 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))
from pcabo import _native as N                                      # noqa: E402

FP64_PEAK = 78.6e12                                                  # FP64 MFMA, MI355X


def seeded_state(n, k, seed=0, relevant=0):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-2.0, 2.0, size=(n, k))
    y = np.sin(3.0 * Z[:, 0]) + 0.5 * (Z[:, :relevant or k] ** 2).sum(1) + 0.1 * rng.standard_normal(n)
    return Z, y


def mll_grad_work(n, k):
    """Work of one k_mll_grad launch: the model counts the lower half of K^-1 = R^T R (n^3/6 multiply-adds = n^3/3 FLOP) and
    the distance recompute (2 n^2 k); `issued` is what the whole 64 x 64 tiles of the launch execute on the MFMAs."""
    NP = -(-n // 64) * 64
    nb, KP = NP // 64, -(-k // 4) * 4
    tiles = [(I, J) for I in range(nb) for J in range(I + 1)]
    issued = sum(2.0 * 64 * 64 * (NP - 64 * I) + 2.0 * 64 * 64 * KP for I, _ in tiles)
    return {"model_flops": n ** 3 / 3.0 + 2.0 * n * n * k, "issued_flops": issued, "tiles": len(tiles)}


def clock(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="450x36,1050x89")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ard", action="store_true", help="also time the fit with one lengthscale per input")
    ap.add_argument("--relevant", type=int, default=0, help="y depends on the first R inputs only (0: all)")
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("needs a HIP device")
    out = []
    for shape in a.shapes.split(","):
        n, k = (int(v) for v in shape.split("x"))
        Z, y = seeded_state(n, k, relevant=a.relevant)
        ctx = N.Context(max_n=n, max_d=k, max_q=64)
        fit = ctx.gp_fit(y, Z=Z)                                       # warm-up (and the fitted theta)
        fit_ms = clock(lambda: ctx.gp_fit(y, Z=Z), a.reps)
        th = fit["theta"]
        mll_ms = clock(lambda: ctx.gp_mll(y, th, Z=Z), 4 * a.reps)
        cond_ms = clock(lambda: ctx.gp_condition(y, Z=Z, lengthscale=fit["lengthscale"], noise=fit["noise"]), 4 * a.reps)
        ard = {}
        if a.ard:
            afit = ctx.gp_fit_ard(y, Z=Z)                              # warm-up (and the fitted theta)
            afit_ms = clock(lambda: ctx.gp_fit_ard(y, Z=Z), max(1, a.reps // 2))
            amll_ms = clock(lambda: ctx.gp_mll_ard(y, afit["theta"], Z=Z), 4 * a.reps)
            ard = {"ard_evaluations_per_fit": afit["evaluations"], "ard_iterations": afit["iterations"], "ard_warnflag": afit["warnflag"],
                   "ard_ms_per_fit": afit_ms, "ard_ms_per_evaluation": afit_ms / max(1, afit["evaluations"]), "ard_ms_gp_mll": amll_ms,
                   "ard_loss": afit["loss"], "scalar_loss": fit["loss"], "relevant": a.relevant,
                   "ard_lengthscale_min": float(afit["lengthscales"].min()), "ard_lengthscale_max": float(afit["lengthscales"].max())}
        ctx.close()
        row = {"n": n, "k": k, "evaluations_per_fit": fit["evaluations"], "iterations": fit["iterations"],
               "warnflag": fit["warnflag"], "ms_per_fit": fit_ms, "ms_per_evaluation": fit_ms / max(1, fit["evaluations"]),
               "ms_gp_mll": mll_ms, "ms_gp_condition": cond_ms, "mll_share_of_evaluation": (mll_ms - cond_ms) / mll_ms,
               **mll_grad_work(n, k), **ard}
        out.append(row)
        print(f"n={n:5d} k={k:3d}: {row['evaluations_per_fit']} evaluations / {row['iterations']} iterations per fit, "
              f"{fit_ms:8.2f} ms per fit, {row['ms_per_evaluation']:6.3f} ms per evaluation (gp_mll alone {mll_ms:6.3f}, "
              f"conditioning alone {cond_ms:6.3f}: marginal-likelihood share {100 * row['mll_share_of_evaluation']:5.1f} %); "
              f"k_mll_grad work {row['issued_flops'] / 1e9:.3f} GFLOP issued = {row['issued_flops'] / FP64_PEAK * 1e6:.1f} us "
              f"at the FP64 MFMA peak", flush=True)
        if ard:
            print(f"             ARD: {ard['ard_evaluations_per_fit']} evaluations / {ard['ard_iterations']} iterations per fit (warnflag "
                  f"{ard['ard_warnflag']}), {ard['ard_ms_per_fit']:8.2f} ms per fit, {ard['ard_ms_per_evaluation']:6.3f} ms per evaluation "
                  f"(gp_mll_ard alone {ard['ard_ms_gp_mll']:6.3f}); loss {ard['ard_loss']:.4f} (scalar fit {ard['scalar_loss']:.4f}), "
                  f"lengthscales {ard['ard_lengthscale_min']:.3g} .. {ard['ard_lengthscale_max']:.3g}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
