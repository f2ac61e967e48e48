"""sha256 of what Context.wpca returns (data_mean, pca_mean, components, evr, k, Z) on seeded inputs at the shapes where
k_jacobi can go wrong: tests/golden/wpca_bits_hashes.json pins the bits of the weighted PCA so that a rewrite of the
eigen-solver's round (lane layout, number of waves, LDS layout, how the rotation flag travels) is held to "same eigenvectors,
eigenvalues, sweep count, components, ratios, k" (tests/test_gpu_wpca_bits.py).  A run's trajectory is chaotic: a last-bit
change here moves the candidates of later iterations at order one.
  grid      d in GRID_D x n in {2, d - 1, d, d + 1, 3 d} (<= 400) x the four generators of tests/wpca_reference.py: a cold
            call, then two warm calls with one row appended each, as in a run (the second depends on the bits of the stored
            eigenvectors).  Odd d (virtual column), every rows-per-lane boundary of 16 (and of 8) lanes per pair, the d = 64 / 65
            split, staged (d <= 64) and unstaged warm start, rcount = n < d, `twin`: tied eigenvalues (tie order of s_order)
  extra     warm after a rank-deficient call and after collapsed start vectors (fallback to cold), data times 2^270 (range
            guard), n_components fixed
  batch     three different runs through Batch.wpca_gp_condition_begin -> wpca_results, cold and warm, next to the same three
            as single calls (no Z: the batch does not return it)
    python tools/gpu_wpca_hashes.py                 # print
    python tools/gpu_wpca_hashes.py --write [FILE]  # regenerate (only after an INTENDED change of arithmetic)
PCABO_LIB selects the library: the golden file was written with the library as it was before k_jacobi's round was rewritten."""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "para-ortho-pca-bo_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import wpca_reference as R

GOLDEN = os.path.join(ROOT, "tests", "golden", "wpca_bits_hashes.json")
GRID_D = (1, 2, 3, 5, 16, 17, 32, 33, 40, 48, 49, 63, 64, 65, 100, 127, 128)
N_CAP = 400
MAX_N, MAX_D = 512, 128
EXTRAS = ("rank-deficient", "scaled", "n-components")
FIELDS = ("data_mean", "pca_mean", "components", "evr")


def grid_n(d):
    out = []
    for n in (2, d - 1, d, d + 1, 3 * d):
        n = min(n, N_CAP)
        if n >= 2 and n not in out:
            out.append(n)
    return out


def digest(res, with_Z=True) -> str:
    h = hashlib.sha256()
    for key in FIELDS + (("Z",) if with_Z else ()):
        h.update(np.ascontiguousarray(res[key], dtype=np.float64).tobytes())
    h.update(np.int64(res["k"]).tobytes())
    return h.hexdigest()[:32]


def force_cold(ctx, d):
    """A two-point call of another d: the next call of dimension d cannot reuse eigenvectors."""
    dd = 2 if d == 1 else 1
    ctx.wpca(np.arange(2.0 * dd).reshape(2, dd), ranks=np.array([1, 2]))


def prefix(case, m):
    """(X, ranks, noise) of the first m points of a case, ranked among themselves."""
    return case.X[:m], R.stable_ranks(case.f[:m]), case.noise[:m]


def run_sequence(ctx, gen, d, n, scale=1.0, **kw):
    """Cold on the first n points of a case of n + 2, then warm on n + 1 and on n + 2: three digests."""
    case = R.make_case(gen, d, n + 2)
    force_cold(ctx, d)
    out = []
    for m in (n, n + 1, n + 2):
        X, ranks, noise = prefix(case, m)
        out.append(digest(ctx.wpca(X * scale, ranks=ranks, noise=noise * scale, **kw)))
    return out


def compute_d(ctx, d) -> dict:
    return {"%s-d%d-n%d" % (gen, d, n): run_sequence(ctx, gen, d, n) for gen in R.GENERATORS for n in grid_n(d)}


def compute_extra(ctx, what) -> dict:
    out = {}
    if what == "rank-deficient":
        for d in (40, 100):
            A = R.make_case("lhs", d, 120)
            force_cold(ctx, d)
            B = R.make_case("cluster", d, 5, salt=2)                       # n < d: null columns are normalised rounding noise
            ctx.wpca(B.X, ranks=B.ranks, noise=B.noise)
            out["after-rank-deficient-d%d" % d] = [digest(ctx.wpca(A.X, ranks=A.ranks, noise=A.noise))]
            Cc = R.make_case("lhs", d, d + 20, salt=3)
            Cc.X[:, d // 2] = 1.25                                         # no noise: a zero-norm eigenvector, rejected as a start
            force_cold(ctx, d)
            rc = ctx.wpca(Cc.X, ranks=Cc.ranks)
            assert np.any((rc["components"] == 0.0).all(axis=1))
            out["after-collapsed-d%d" % d] = [digest(rc), digest(ctx.wpca(A.X, ranks=A.ranks, noise=A.noise))]
    elif what == "scaled":
        for d in (40, 100):
            out["scaled-2^270-d%d" % d] = run_sequence(ctx, "cluster", d, 120, scale=2.0 ** 270)
    elif what == "n-components":
        out["n-components-7-d40"] = run_sequence(ctx, "lhs", 40, 120, n_components=7)
        out["n-components-70-d100"] = run_sequence(ctx, "twin", 100, 150, n_components=70)
    else:
        raise ValueError(what)
    return out


BATCH_RUNS = (("lhs", 0), ("cluster", 1), ("twin", 2))
BATCH_D, BATCH_N = 40, 60


def compute_batch(N) -> dict:
    """{"batch": [cold b0..b2, warm b0..b2], "single": the same from three contexts of their own}."""
    cases = [R.make_case(g, BATCH_D, BATCH_N + 1, salt=s) for g, s in BATCH_RUNS]
    bt = N.Batch(len(cases), max_n=MAX_N, max_d=BATCH_D, max_q=64)
    singles = [N.Context(max_n=MAX_N, max_d=BATCH_D, max_q=64) for _ in cases]
    out = {"batch": [], "single": []}
    rng = np.random.default_rng(11)
    for m in (BATCH_N, BATCH_N + 1):
        parts = [prefix(c, m) for c in cases]
        X, ranks, noise = (np.stack([p[i] for p in parts]) for i in range(3))
        y = np.stack([c.f[:m] for c in cases])
        bt.wpca_gp_condition_begin(X, ranks, noise, y)
        res = bt.wpca_results()
        out["batch"] += [digest(r, with_Z=False) for r in res]
        _, st = bt.gp_wait_eval([rng.uniform(-1.0, 1.0, size=(32, r["k"])) for r in res], y.min(axis=1))
        assert not st.any()
        out["single"] += [digest(c.wpca(*p[:1], ranks=p[1], noise=p[2]), with_Z=False) for c, p in zip(singles, parts)]
    bt.close()
    for c in singles:
        c.close()
    return out


def compute() -> dict:
    from pcabo import _native as N
    ctx = N.Context(max_n=MAX_N, max_d=MAX_D, max_q=64)
    out = {}
    for d in GRID_D:
        out.update(compute_d(ctx, d))
    for what in EXTRAS:
        out.update(compute_extra(ctx, what))
    ctx.close()
    out.update(compute_batch(N))
    return out


if __name__ == "__main__":
    res = compute()
    if "--write" in sys.argv:
        i = sys.argv.index("--write")
        dst = sys.argv[i + 1] if len(sys.argv) > i + 1 else GOLDEN
        with open(dst, "w") as f:
            json.dump({"_comment": "tools/gpu_wpca_hashes.py --write on an MI355X, with the library as it was before the round of "
                                   "k_jacobi was rewritten (16 lanes per pair everywhere, flag through a flat store)", "cases": res},
                      f, indent=0)
        print("written", dst, len(res), "entries")
    else:
        print(json.dumps(res, indent=0))
