"""sha256 of what Context.optimize_acqf returns - candidates, values and the info rows (iterations, evaluations, warnflag, task) - on
every path the call can take through its round loop, on two small seeded GP states (k = 3, Matern-5/2, n = 64: NP = 64 and
n = 65: NP = 128):
  r5        5 restarts             one group: no helper thread
  r7_l5     7 restarts, limit 5    two uneven groups: the free-running pair on the resident kernel
  r12_l5    12 restarts, limit 5   three groups: lock-step rounds through the resident kernel
  r32_l2    32 restarts, limit 2   16 groups, three stepping threads (resident at n = 64 only: the grid must fit the chip)
  r60_l5    60 restarts, limit 5   12 groups, plain launches (more queries than the resident kernel takes)
each with PCABO_OPT_RESIDENT 1 (`resident`) and 0 (`launches`), r7_l5 and r12_l5 also with PCABO_OPT_GROUP_ACQ (`group`).
Whether a call really takes the resident kernel depends on the machine (another process on the device, a slow first answer); the
bits must not, which is what tests/test_gpu_optimize_paths_bits.py pins.  tests/golden/optimize_paths_hashes.json holds the bits
of the library before the host side of the call moved into host_side.h (PCABO_LIB selects the library).
    python tools/gpu_optimize_hashes.py            # print
    python tools/gpu_optimize_hashes.py --write    # regenerate (only after an INTENDED change of arithmetic)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "optimize_paths_hashes.json")
NS = (64, 65)
K = 3
SHAPES = {"r5": (5, 5), "r7_l5": (7, 5), "r12_l5": (12, 5), "r32_l2": (32, 2), "r60_l5": (60, 5)}   # restarts, batch limit
MODES = ("resident", "launches", "group")
MAX_Q = 64


def modes_of(shape):
    return MODES if shape in ("r7_l5", "r12_l5") else MODES[:2]


def make_state(n):
    """(Z, y, u): training points, a smooth y on them and the MAX_Q start points as fractions of the search box."""
    rng = np.random.default_rng(7000 + n)
    Z = rng.uniform(-1.0, 1.0, size=(n, K))
    y = ((Z - 0.3) ** 2).sum(1) + np.sin(3.0 * Z[:, 0]) * np.cos(2.0 * Z[:, 1]) + 0.5 * Z[:, 2]
    return Z, y, rng.uniform(0.0, 1.0, size=(MAX_Q, K))


def open_state(N, n):
    """(context conditioned on state n, search box, start points, incumbent)"""
    Z, y, u = make_state(n)
    ctx = N.Context(max_n=n, max_d=K, max_q=MAX_Q)
    ctx.gp_condition(y, Z=Z, kernel=N.KERNEL_MATERN52)
    box = ctx.acq_bounds()
    return ctx, box, box[0] + u * (box[1] - box[0]), float(y.min())


def set_mode(N, ctx, mode):
    ctx.set_option(N.OPT_RESIDENT, 1 if mode == "resident" else 0)
    ctx.set_option(N.OPT_GROUP_ACQ, 1 if mode == "group" else 0)


def optimize(ctx, box, ics, best_f, limit):
    cand, vals, info, _ = ctx.optimize_acqf(ics, box, best_f, batch_limit=limit)
    return cand, vals, info


def digest(cand, vals, info) -> dict:
    assert np.isfinite(cand).all() and np.isfinite(vals).all()
    return {"cand": hashlib.sha256(np.ascontiguousarray(cand, dtype=np.float64).tobytes()).hexdigest(),
            "vals": hashlib.sha256(np.ascontiguousarray(vals, dtype=np.float64).tobytes()).hexdigest(),
            "info": hashlib.sha256(np.ascontiguousarray(info, dtype=np.int32).tobytes()).hexdigest()}


def compute_state(n) -> dict:
    from pcabo import _native as N
    ctx, box, ics, best_f = open_state(N, n)
    out = {}
    for shape, (nr, limit) in SHAPES.items():
        out[shape] = {}
        for mode in modes_of(shape):
            set_mode(N, ctx, mode)
            out[shape][mode] = digest(*optimize(ctx, box, ics[:nr], best_f, limit))
    ctx.close()
    return out


def compute() -> dict:
    return {"n%d" % n: compute_state(n) for n in NS}


if __name__ == "__main__":
    res = compute()
    if "--write" in sys.argv:
        i = sys.argv.index("--write")
        out = sys.argv[i + 1] if len(sys.argv) > i + 1 else GOLDEN
        with open(out, "w") as f:
            json.dump({"_comment": "tools/gpu_optimize_hashes.py --write on an MI355X, with the library as it was before the host side "
                                   "of pcabo_optimize_acqf moved into host_side.h", "cases": res}, f, indent=1)
        print("written", out)
    else:
        print(json.dumps(res, indent=1))
