"""The weighted-PCA kernels (`kernels_wpca.hip`) against an extended-precision reference at edge shapes.

Every result is judged in the error units of `wpca_reference` (first-order analysis of any fp64 implementation;
`test_wpca_reference_cpu.py` shows numpy + sklearn/LAPACK staying under 4 of each).  The device sums in other
orders - LDS trees, a four-wave split MFMA contraction, rcp / rsq + Newton rotations - so its constants may
differ by small factors: the acceptance limit is 16 in every unit.  The defects these tests are there for (a
leaked pad row, a dropped row of n4, a sweep that stops at the 1e-8 test, a wrong pairing for odd d) are >= 1e6.

A call is COLD when the preceding call on the context had another d (a tiny call of another d forces that:
`k_jacobi` then starts from C), WARM when it repeats d (`k_jacobi` starts from C V0, V0 = the previous vectors).
"""
import time

import numpy as np
import pytest

import pcabo_oracle as O
import wpca_reference as R

pytestmark = pytest.mark.gpu

LIMIT = 16.0
EPS = R.EPS
_REFS = {}


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=1050, max_d=128)
    t0 = time.time()
    yield c
    c.close()
    print("\ntest_gpu_wpca_edges: %.1f s between context creation and close" % (time.time() - t0))


def _ref(case):
    """Extended-precision reference of a case, computed once per module run."""
    if case.id not in _REFS:
        _REFS[case.id] = R.reference(case.X, case.ranks, case.noise)
    return _REFS[case.id]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _force_cold(ctx, d):
    """A two-point call of another d: the next call of dimension d cannot reuse eigenvectors."""
    dd = 2 if d == 1 else 1
    ctx.wpca(np.arange(2.0 * dd).reshape(2, dd), ranks=np.array([1, 2]))


def _run(ctx, case, cold=True, **kw):
    if cold:
        _force_cold(ctx, case.d)
    return ctx.wpca(case.X, ranks=case.ranks, noise=case.noise, **kw)


def _judge(case, ref, res, worst, fails, tag="", k_forced=None):
    """Checks of part (a) on one device result; appends (case, what, figure) to `fails`."""
    cid = case.id + tag
    inv = R.judge(ref, res["data_mean"], res["pca_mean"], res["components"], res["evr"])
    for q in R.QUANTITIES:
        v = getattr(inv, q)
        worst.add(case.gen, q, v, cid)
        if not v <= LIMIT:
            fails.append((cid, q, v))
    for flag in ("finite", "evr_monotone", "sign_ok", "dead_ok"):
        if not getattr(inv, flag):
            fails.append((cid, flag, False))
    k_ref = k_forced if k_forced else O.select_components(ref.rho / ref.rho.sum(), 0.95, 0)
    if res["k"] != k_ref:
        fails.append((cid, "k", (res["k"], k_ref)))
    k = res["k"]
    if res["Z"].shape != (case.n, k):
        fails.append((cid, "Z.shape", res["Z"].shape))
        return inv
    Zr, unit = R.project_reference(case.X, res["data_mean"], res["pca_mean"], res["components"][:k])
    dz = np.abs(R.f64(R.hp(res["Z"]) - Zr))
    if np.any(dz[unit == 0.0] != 0.0) or not np.all(np.isfinite(res["Z"])):
        fails.append((cid, "Z (zero unit / not finite)", float(dz.max())))
    zr = float((dz[unit > 0.0] / unit[unit > 0.0]).max()) if np.any(unit > 0.0) else 0.0
    worst.add(case.gen, "Z", zr, cid)
    if not zr <= LIMIT:
        fails.append((cid, "Z", zr))
    return inv


def _report(capsys, worst, title):
    with capsys.disabled():
        print("\n" + worst.table(title))


# ---- a. the grid against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", R.GENERATORS)
def test_grid_cold_against_reference(ctx, gen, capsys):
    """Every grid case, cold, ranks passed as the product passes them.  What each part of the grid is there for:

    - odd d (3, 5, 7, 17, 33, 63, 65, 127): the virtual empty Jacobi column, LD = d | 1 == d;
    - d % 16 != 0: the zero padding of Wc to DP must not leak into C (`k_wpca_prep`, `k_cov`);
    - d = 1, 2 and 63 / 64 / 65: smallest problems and the `k_jacobi<4>` / `<8>` boundary;
    - d in 65 .. 128: CP = 128 in `k_wpca_prep`, 8 lanes per pair above 64 pairs;
    - n % 4 != 0 (n4 rows of `k_cov`) and n % 8 != 0 (last `k_project` block);
    - n = 513, 1050 (d <= 64) and n = 257 .. 1050 (d > 64): the streaming path of `k_wpca_prep`;
    - n <= d (n = 2, 3, 5, d): rcount = n, rank-deficient C - non-live rows need only be finite, norm <= 1;
    - `twin`: exactly paired eigenvalues, `cluster`: eigenvalues down to 1e-12 of the largest - judged by
      residuals, not vector by vector; `shifted`: X ~ 1e3 +- 5e-3, the centring loses ~1e5 eps.

    k must equal select_components on the reference's eigenvalues (no cumulative ratio lies within 1e-9 of the
    threshold, asserted by the CPU file), Z is checked against the projection formed in extended precision from
    the device's own means and components (isolates `k_project`)."""
    worst, fails, skipped = R.Worst(), [], []
    cases = [c for c in R.grid_cases() if c[0] == gen]
    for g, d, n in cases:
        case = R.make_case(g, d, n)
        ref = _ref(case)
        if ref.skip:                                   # (only where long double is a plain double: the large cases)
            skipped.append(case.id)
            continue
        _judge(case, ref, _run(ctx, case), worst, fails)
    _report(capsys, worst, "device / reference units, cold grid, %s (%d cases, %d without a reference)"
            % (gen, len(cases), len(skipped)))
    assert not fails, (len(fails), fails[:30])
    assert R.EXTENDED or len(skipped) < len(cases)
    assert not (R.EXTENDED and skipped)


# ---- b. warm equals cold ---------------------------------------------------------------------------------------------
def _agree(case, ref, ra, rb, what, worst, fails):
    """Live components of two runs agree to 16 T / gap_r (rows with gap_r < 1e3 T are left to the residuals)."""
    gap = R.gaps(ref)
    live = (ref.rho > 1e3 * ref.T) & (gap >= 1e3 * ref.T)
    if ra["k"] != rb["k"]:
        fails.append((case.id, what + " k", (ra["k"], rb["k"])))
    a, b = ra["components"][live], rb["components"][live]
    if a.size == 0:
        return
    diff = np.minimum(np.sqrt(((a - b) ** 2).sum(axis=1)), np.sqrt(((a + b) ** 2).sum(axis=1)))
    unit = ref.T / gap[live]                           # (d = 1: no other eigenvalue, unit 0 - the vector is exactly [1])
    ratio = float(np.where(unit > 0.0, diff / np.where(unit > 0.0, unit, 1.0), 0.0).max())
    worst.add(case.gen, "warm-cold", ratio, case.id + " " + what)
    if not np.all(diff <= LIMIT * unit):
        fails.append((case.id, what, ratio))


@pytest.mark.parametrize("gen", ("lhs", "cluster"))
def test_warm_start_equals_cold_start(ctx, gen, capsys):
    """`k_jacobi` "does not depend on the start beyond rounding": A cold, then an UNRELATED case B of the same d
    (the context reuses B's vectors whatever data they came from), then A warm from B's vectors, then A warm from
    its own.  All three A results pass part (a), k is identical, live components agree to 16 T / gap.  Every d of
    the grid at n = 120 and n = 450: d <= 64 stages C and V0 in LDS, d = 65, 100, 127, 128 reads them from global
    memory (the column-of-C read that relies on C being symmetric bit for bit)."""
    other = "cluster" if gen == "lhs" else "lhs"
    worst, fails = R.Worst(), []
    for d in R.GRID_D:
        for n in (120, 450):
            A, B = R.make_case(gen, d, n), R.make_case(other, d, n, salt=1)
            ref = _ref(A)
            if ref.skip:
                pytest.skip(ref.skip)
            r_cold = _run(ctx, A)
            _run(ctx, B, cold=False)
            r_warm_b = _run(ctx, A, cold=False)
            r_warm_a = _run(ctx, A, cold=False)
            for tag, r in ((" cold", r_cold), (" warm<-B", r_warm_b), (" warm<-A", r_warm_a)):
                _judge(A, ref, r, worst, fails, tag)
            _agree(A, ref, r_cold, r_warm_b, "cold vs warm<-B", worst, fails)
            _agree(A, ref, r_cold, r_warm_a, "cold vs warm<-A", worst, fails)
    _report(capsys, worst, "device / reference units, warm start, %s" % gen)
    assert not fails, (len(fails), fails[:30])


@pytest.mark.parametrize("d", (40, 100))
def test_warm_start_after_rank_deficient_or_collapsed_vectors(ctx, d, capsys):
    """The previous call's vectors are not a basis the warm start may trust:

    - B with n < d: its null columns of G = C V are normalised rounding noise (unit norm, so the warm-start test
      accepts them) - A started from them must still pass part (a) and agree with the cold run;
    - B with a constant column and no noise: that column of C is exactly zero, its eigenvector has norm 0, and the
      next call must silently fall back to the cold start - the SAME bits as the cold run."""
    worst, fails = R.Worst(), []
    A = R.make_case("lhs", d, 120)
    ref = _ref(A)
    if ref.skip:
        pytest.skip(ref.skip)
    r_cold = _run(ctx, A)
    _run(ctx, R.make_case("cluster", d, 5, salt=2), cold=False)               # n < d
    r_warm = _run(ctx, A, cold=False)
    _judge(A, ref, r_cold, worst, fails, " cold")
    _judge(A, ref, r_warm, worst, fails, " warm<-rank-deficient")
    _agree(A, ref, r_cold, r_warm, "cold vs warm<-rank-deficient", worst, fails)

    B = R.make_case("lhs", d, d + 20, salt=3)
    B.X[:, d // 2] = 1.25
    _force_cold(ctx, d)                                                       # (from C itself the zero column stays zero)
    rb = ctx.wpca(B.X, ranks=B.ranks)                                         # no noise: column d/2 of C is 0.0
    assert np.any((rb["components"] == 0.0).all(axis=1)), "B was meant to leave a zero-norm eigenvector"
    r_fall = _run(ctx, A, cold=False)
    for key in ("data_mean", "pca_mean", "components", "evr", "Z"):
        if not _same_bits(r_cold[key], r_fall[key]):
            fails.append((A.id, "fallback to cold start: bits of " + key, float(np.abs(r_cold[key] - r_fall[key]).max())))
    if r_cold["k"] != r_fall["k"]:
        fails.append((A.id, "fallback k", (r_cold["k"], r_fall["k"])))
    _report(capsys, worst, "device / reference units, warm start after unusable vectors, d = %d" % d)
    assert not fails, fails


# ---- c. streaming path of k_wpca_prep -------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n_regs,n_stream", [(40, 512, 516), (40, 509, 513), (100, 256, 260), (100, 253, 257)])
def test_streaming_path_matches_register_path(ctx, d, n_regs, n_stream, capsys):
    """`k_wpca_prep` keeps a thread's rows in registers while (n4 + G - 1) / G <= 32 and streams through Wc beyond
    (d <= 64: n4 <= 512, d > 64: n4 <= 256); its comment claims the same bits.  Which path runs depends on n and d
    alone - not on the context's capacity - so no n runs both and the bit claim REMAINS UNVERIFIED; what is checked
    is that the last register-path n and the first streaming n (also with n % 4 != 0) both pass part (a) against the
    reference, with the reference's pattern of live rows on both sides."""
    worst, fails = R.Worst(), []
    for gen in ("lhs", "cluster", "shifted"):
        patterns = []
        for n in (n_regs, n_stream):
            case = R.make_case(gen, d, n)
            ref = _ref(case)
            if ref.skip:
                pytest.skip(ref.skip)
            inv = _judge(case, ref, _run(ctx, case), worst, fails)
            if not np.array_equal(inv.live, ref.rho > 1e3 * ref.T):
                fails.append((case.id, "live rows differ from the reference's", int(inv.live.sum())))
            patterns.append(inv.live)
        if gen == "lhs" and not np.array_equal(patterns[0], patterns[1]):
            fails.append((gen, "live pattern differs between the paths", None))
    _report(capsys, worst, "device / reference units, register vs streaming path, d = %d" % d)
    assert not fails, fails


# ---- d. the power-of-four range guard -------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ("cold", "warm"))
@pytest.mark.parametrize("d", (7, 40, 100))
@pytest.mark.parametrize("gen", ("lhs", "cluster"))
def test_range_guard_commutes_with_a_power_of_four(ctx, gen, d, start):
    """`k_jacobi` scales C by a power of four when its largest entry leaves 2^+-100 and promises that every
    operation of the sweep commutes with that factor exactly.  (X, noise) times 2^200 and times 2^-200 (C times
    2^+-400: the guard fires both ways) must give bit-identical k, evr and components and exactly scaled means and
    Z.  Each call starts from the same state: cold (G = C cscale), or warm from the vectors of one fixed case B
    (G = (C cscale) V0, the staged and the global-memory variant)."""
    A, B = R.make_case(gen, d, 120), R.make_case("lhs", d, 31, salt=4)
    out = []
    for e in (0, 200, -200):
        s = 2.0 ** e
        _force_cold(ctx, d)
        if start == "warm":
            _run(ctx, B, cold=False)
        out.append((s, ctx.wpca(A.X * s, ranks=A.ranks, noise=A.noise * s)))
    (_, r0) = out[0]
    assert np.all(np.isfinite(r0["components"])) and np.all(np.isfinite(r0["Z"]))
    for s, r in out[1:]:
        assert r["k"] == r0["k"], (s, r["k"], r0["k"])
        for key in ("evr", "components"):
            assert _same_bits(r[key], r0[key]), (s, key, float(np.abs(r[key] - r0[key]).max()))
        for key in ("data_mean", "pca_mean", "Z"):
            assert _same_bits(r[key], r0[key] * s), (s, key, float(np.abs(r[key] / s - r0[key]).max()))


# ---- e. ranking with ties --------------------------------------------------------------------------------------------
def _tied_f(n, kind, rng):
    if kind == "all-equal":
        return np.full(n, 3.5)
    f = rng.normal(size=n)
    f[rng.random(n) < 0.4] = 1000.0                    # every out-of-box evaluation is exactly 1000.0
    f[: max(1, n // 4)] = f[0]                         # a block of equal ordinary values
    if n >= 5:
        f[n // 2], f[n // 2 + 1] = 0.0, -0.0           # equal, different bits
        f[-1] = 1000.0
    else:
        f[0], f[1] = 0.0, -0.0
    return f


@pytest.mark.parametrize("maximize", (False, True))
@pytest.mark.parametrize("kind", ("blocks", "all-equal"))
@pytest.mark.parametrize("n", (2, 5, 64, 257, 450))
def test_device_ranking_with_ties(ctx, n, kind, maximize):
    """`k_rank`: ties broken by index, also under `maximize` and for 0.0 / -0.0 - wpca(f=...) must equal
    wpca(ranks=stable_ranks(f)) bit for bit in every output (n = 257, 450: more than one block of `k_rank`)."""
    d = 6
    rng = np.random.default_rng([n, int(maximize), 77])
    X, noise = rng.uniform(-5.0, 5.0, size=(n, d)), rng.normal(0.0, 1e-8, size=(n, d))
    f = _tied_f(n, kind, rng)
    assert len(set(f.tolist())) < n
    _force_cold(ctx, d)
    a = ctx.wpca(X, f=f, maximize=maximize, noise=noise)
    _force_cold(ctx, d)
    b = ctx.wpca(X, ranks=R.stable_ranks(f, maximize), noise=noise)
    assert a["k"] == b["k"]
    for key in ("data_mean", "pca_mean", "components", "evr", "Z"):
        assert _same_bits(a[key], b[key]), (key, float(np.nanmax(np.abs(a[key] - b[key]))))
    if kind == "blocks":                               # the tie order matters: the reversed one gives other weights
        _force_cold(ctx, d)
        rev = n + 1 - R.stable_ranks(-f if not maximize else f, False)
        c = ctx.wpca(X, ranks=rev, noise=noise)
        assert not _same_bits(a["pca_mean"], c["pca_mean"])


# ---- f. rows D, E, J, O ----------------------------------------------------------------------------------------------
def test_bounds_statistics_and_inverse_map(ctx, capsys):
    """`k_zstats` and `k_inverse_map` on the grid cases with n in {31, 450}, n > d, n_components forced to the
    number of live components: k up to 128 (CP = 128 in `k_zstats` for k > 64), k % 8 != 0 (the remainder loop
    behind the `c + 8 <= k` loop of `k_inverse_map`), n = 31 (only the remainder of the 8-way unrolled loop of
    `k_zstats`) and n = 450 (both), boxes narrower than 0.1 (`shifted`, the small components of `cluster`) and
    wider.  norm_bounds / acq_bounds against oracle.normalize_bounds / acq_bounds of the device's Z to
    4 eps max(|zmin|, |zmax|, |rng|); y_mean, y_std and inverse_map against extended precision, limit 16.
    `k_znorm` has no getter: gp_condition() runs it, nothing here reads its output (`test_gpu_gp_edges.py` judges it
    through K).

    The round trip inverse_map(Z[i]) ~ X[i] is NOT checked: its bound sqrt(sum_dead rho) sqrt(n / w_min) is
    infinite, the worst-ranked point has weight ln n - ln n = 0."""
    worst, fails = R.Worst(), []
    narrow = wide = 0
    ks = set()
    for gen, d, n in R.grid_cases():
        if n not in (31, 450) or n <= d:
            continue
        case = R.make_case(gen, d, n)
        ref = _ref(case)
        if ref.skip:
            pytest.skip(ref.skip)
        k = int((ref.rho > 1e3 * ref.T).sum())
        res = _run(ctx, case, n_components=k)
        _judge(case, ref, res, worst, fails, " k=%d" % k, k_forced=k)
        if res["k"] != k:
            continue
        ks.add(k)
        rng = np.random.default_rng([R.GENERATORS.index(gen), d, n, 5])
        y = rng.normal(size=n) * 10.0 ** rng.uniform(-2, 3) + rng.normal() * 10.0
        ctx.gp_condition(y)
        st = ctx.gp_state()
        Z = res["Z"]
        zmin, zmax = Z.min(axis=0), Z.max(axis=0)
        unit = 4.0 * EPS * np.maximum(np.maximum(np.abs(zmin), np.abs(zmax)), zmax - zmin)
        for name, dev, want in (("norm_bounds", st["norm_bounds"], O.normalize_bounds(Z)),
                                ("acq_bounds", ctx.acq_bounds(), O.acq_bounds(Z))):
            err = np.abs(dev - want)
            if not np.all(err <= unit[None, :]):
                fails.append((case.id, name, float((err / unit[None, :]).max())))
        ab = O.acq_bounds(Z)
        widened = (zmax + 0.5 * (zmax - zmin)) - (zmin - 0.5 * (zmax - zmin)) < 0.1
        narrow += int(widened.sum())
        wide += int((~widened).sum())
        yh = R.hp(y)
        ym = yh.sum() / n
        ysd = R.hp_sqrt(((yh - ym) ** 2).sum() / (n - 1))
        r_mean = abs(float(R.hp(st["y_mean"]) - ym)) / (n * EPS * np.abs(y).mean())
        r_std = abs(float(R.hp(st["y_std"]) - ysd)) / (n * EPS * float(ysd))
        worst.add(gen, "y_mean", r_mean, case.id)
        worst.add(gen, "y_std", r_std, case.id)
        if not r_mean <= LIMIT:
            fails.append((case.id, "y_mean", r_mean))
        if not r_std <= LIMIT:
            fails.append((case.id, "y_std", r_std))
        ck = res["components"][:k]
        zs = [Z[0], Z[n - 1], ab[0] + rng.random(k) * (ab[1] - ab[0])]
        for z in zs:
            x = ctx.inverse_map(z)
            xr, ux = R.inverse_reference(z, res["data_mean"], res["pca_mean"], ck)
            r_inv = float((np.abs(R.f64(R.hp(x) - xr)) / ux).max())
            worst.add(gen, "inverse", r_inv, case.id)
            if not r_inv <= LIMIT:
                fails.append((case.id, "inverse_map", r_inv))
    _report(capsys, worst, "device / reference units, rows D, E, J, O (k forced to the live count)")
    with capsys.disabled():
        print("  k values: %s\n  acquisition boxes widened to 0.1: %d, left alone: %d" % (sorted(ks), narrow, wide))
    assert narrow > 0 and wide > 0
    assert max(ks) > 64 and any(k % 8 for k in ks) and any(k >= 8 and k % 8 == 0 for k in ks)
    assert not fails, (len(fails), fails[:30])
