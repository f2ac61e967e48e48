"""The native clocks of Context.propose_acqf at the benchmark's shape, with and without the early wake-up of the stepping helper -
diagnostic.  usage: gpu_propose_clock.py [n] [k] [repetitions] [maxiter]
Every repetition conditions the GP anew (enqueued only, as a BO iteration does) and proposes from 512 raw samples, 10 restarts in
groups of 5; wake-up on and off alternate.  With a small maxiter (default 2) the optimise clock is a few rounds long, so what the
helper's wake-up costs in front of the first round is not lost in the rounds' own spread.  The fourth column is the library's own
clock around the call's first advance_all (every group's first L-BFGS-B step; the helper must be awake to take its share).
Prints quartiles in microseconds."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))
import numpy as np
import torch
from pcabo import _native as N
torch.set_num_threads(4)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
k = int(sys.argv[2]) if len(sys.argv) > 2 else 12
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 400
maxiter = int(sys.argv[4]) if len(sys.argv) > 4 else 2
rng = np.random.default_rng(1)
Z = rng.uniform(-2.0, 2.0, (n, k))
y = rng.normal(size=n) * 30.0 + 100.0
raw = rng.uniform(-2.0, 2.0, (512, k))
ctx = N.Context(max_n=n, max_d=k, max_q=512)
N.LIB.pcabo_debug_first_advance_seconds.argtypes = [ctypes.c_void_p]
N.LIB.pcabo_debug_first_advance_seconds.restype = ctypes.c_double
torch.manual_seed(3)
clocks = {True: [], False: []}
for rep in range(reps + 20):
    wake = rep % 2 == 0
    blob = torch.get_rng_state().numpy()
    ctx.gp_condition(y, Z=Z, wait=False)
    box = ctx.acq_bounds()
    r = ctx.propose_acqf(raw, blob, 10, box, float(y.min()), batch_limit=5, maxiter=maxiter, wake=wake)
    torch.set_rng_state(torch.from_numpy(blob))
    if rep >= 20 and r["picked"]:
        clocks[wake].append(np.append(r["phase_seconds"], N.LIB.pcabo_debug_first_advance_seconds(ctx._h)) * 1e6)
ctx.close()
out = {"n": n, "k": k, "maxiter": maxiter, "repetitions_each": len(clocks[True]), "columns_us": ["wait + score", "pick", "optimise", "first advance_all"]}
for w, c in clocks.items():
    q = np.percentile(np.array(c), [25, 50, 75], axis=0)
    out["wake" if w else "asleep"] = {name: [round(float(v), 2) for v in row] for name, row in zip(("q25", "median", "q75"), q)}
print(json.dumps(out))
