"""The GP conditioning kernels against an extended-precision reference at edge shapes.

`k_zstats`, `k_znorm`, `k_gram`, the Cholesky kernels (`k_chol_step`, `k_chol_panel_m`, `k_chol_lookn`,
`k_chol_lookback`), `k_trinv_diag_w`, `k_trinv_cols`, `k_rmatvec` and `k_rtmatvec` are judged in the error units of
`gp_reference` (first-order analysis of any fp64 implementation; `test_gp_reference_cpu.py` shows a numpy
restatement staying under 4 of each and wrong variants leaving them).  The device sums in other orders - MFMA
chains, 64-wide panels, rsq + Newton pivots, a 16-wave split mat-vec - so its constants may differ by small
factors: the acceptance limit is 16 in every unit, as in `test_gpu_wpca_edges.py`.

`k_znorm` has no getter: its output (the normalised, centred, scaled points and their norms) is tested THROUGH K,
whose unit contains nothing else that is large - a wrong row, a leaked pad column or a wrong mean shows there.

One context of capacity 321 x 128 serves every case, large problems first: the leading dimension exceeds the padded
size almost everywhere and every small problem meets the remains of a larger one.  L and R are read WITHOUT the
`np.tril` of `Context.gp_state()`, so their strict upper triangles are checked too.
"""
import ctypes as C
import time

import numpy as np
import pytest

import gp_reference as G

pytestmark = pytest.mark.gpu

LIMIT = 16.0
BIG_N, BIG_D = 321, 128
_REFS = {}


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=BIG_N, max_d=BIG_D, max_q=16)
    t0 = time.time()
    yield c
    c.close()
    print("\ntest_gpu_gp_edges: %.1f s between context creation and close" % (time.time() - t0))


def _ref(case):
    """Extended-precision reference of a case, computed once per module run and never modified."""
    if case.id not in _REFS:
        _REFS[case.id] = G.reference(case)
    return _REFS[case.id]


def _condition(native, c, case):
    c.gp_condition(case.y, Z=case.Z, norm_bounds=case.norm_bounds, lengthscale=case.lengthscale, noise=case.noise,
                   kernel=native.KERNEL_RBF if case.kernel == "rbf" else native.KERNEL_MATERN52)


def _raw_state(native, c):
    """pcabo_get_gp_state as it is: the full n x n blocks of L and R, upper triangles included."""
    n, k = c.n, c.k
    L, R, alpha, ys, nb = np.empty((n, n)), np.empty((n, n)), np.empty(n), np.empty(2), np.empty((2, k))
    ptr = [a.ctypes.data_as(C.c_void_p) for a in (L, R, alpha, ys, nb)]
    c._chk(native.LIB.pcabo_get_gp_state(c._h, *ptr))
    return {"L": L, "R": R, "alpha": alpha, "y_mean": ys[0], "y_std": ys[1], "norm_bounds": nb}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _judge(native, c, case, worst, fails):
    ref = _ref(case)
    _condition(native, c, case)
    st, K = _raw_state(native, c), c.gram()
    j = G.judge(ref, K, st["L"], st["R"], st["alpha"], case.y, st["y_mean"], st["y_std"], st["norm_bounds"])
    for q in G.QUANTITIES:
        v = getattr(j, q)
        worst.add(case.gen, q, v, case.id)
        if not v <= LIMIT:
            fails.append((case.id, q, v))
    for flag in G.FLAGS:
        if not getattr(j, flag):
            fails.append((case.id, flag, False))
    return st


def _report(capsys, worst, title, t0):
    with capsys.disabled():
        print("\n" + worst.table(title) + "\n  %.1f s" % (time.time() - t0))


# ---- a. the grid against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("part", G.GRID_PARTS)
@pytest.mark.parametrize("gen", G.GENERATORS)
def test_grid_against_reference(native, ctx, gen, part, capsys):
    """Default hyperparameters (Matern-5/2, ln 2, e^-5).  What each part of the grid is there for:

    - n = 2, 3, 16, 17: one tile, almost all of it identity padding (`k_gram`'s `i >= n || j >= n` branch, the panel
      kernel factoring the padding, `k_rmatvec` rows with i < 64 only, the remainder loop of `k_rtmatvec` alone);
    - n = 63 / 64 / 65, 127 / 128 / 129, 192 / 193: no padding, one row of padding short of a tile, one row INTO the
      next tile (63 rows of padding) - nblk = 1 .. 4, the first look-ahead group of `k_chol_step` at nblk = 3, the
      first off-diagonal step of `k_trinv_cols` at nblk = 2 and its K loop at nblk >= 3;
    - n = 257, 321: nblk = 5, 6 - both operand sets of the look-ahead in use, `k_rtmatvec`'s unrolled loop;
    - k = 1, 5, 33 and 2, 3, 4, 8, 64, 65, 128 at n = 65, 129: KP = k rounded up to 4 (zero rows of AT for
      k % 4 != 0, clamped loads in `k_znorm`), k = 1 alone, CP = 128 in `k_zstats` above k = 64;
    - `cluster`: three quarters of the points within 1e-3 of the range - the norm + GEMM distance cancels;
      `twins`: exact duplicates, also (i, i + 65) across a tile boundary; `shifted`: columns at 1e3 +- 5e-3 with
      scales from 1e-6 to 1e6, which Normalize has to remove.

    Per case, in units: K of `gram()` against the reference K; |L L^T - K|, |L R - I|, |K alpha - y_s| evaluated in
    extended precision; alpha against the reference alpha; diag(R) diag(L) - 1; the Normalize bounds.  Exactly:
    K symmetric, the strict upper triangles of L and R zero, diag(L) > 0."""
    t0 = time.time()
    worst, fails, skipped = G.Worst(), [], []
    sizes = G.grid_part(part)
    assert sizes[0][0] >= 129 and sizes[-1][0] <= 65           # small problems follow large ones
    for n, k in sizes:
        case = G.make_case(gen, n, k)
        if _ref(case).skip:                            # (only where long double is a plain double)
            skipped.append(case.id)
            continue
        _judge(native, ctx, case, worst, fails)
    _report(capsys, worst, "device / reference units, %s, %s (%d cases, %d without a reference)"
            % (gen, part, len(sizes), len(skipped)), t0)
    assert not fails, (len(fails), fails[:30])
    assert not (G.EXTENDED and skipped) and len(skipped) < len(sizes)


@pytest.mark.parametrize("gen", G.GENERATORS)
def test_hyperparameter_sets_against_reference(native, ctx, gen, capsys):
    """n = 65, 129, 193, k = 1, 5: Matern with lengthscale 0.05 and noise 1e-6 (u_K at its widest, entries of K, L and
    R down to the underflow range); RBF with lengthscale 3 and noise 1e-4 (condition number ~1e6: the kappa terms of
    the alpha units carry the judgement); Matern with user bounds wider than the data (the `user_nb` branch of
    `k_zstats`, which `gp_state()` must hand back unchanged)."""
    t0 = time.time()
    worst, fails = G.Worst(), []
    for n, k, hyper in G.hyper_sizes():
        case = G.make_case(gen, n, k, hyper)
        if _ref(case).skip:
            pytest.skip(_ref(case).skip)
        st = _judge(native, ctx, case, worst, fails)
        if case.norm_bounds is not None and not _same_bits(st["norm_bounds"], case.norm_bounds):
            fails.append((case.id, "user bounds changed", None))
    _report(capsys, worst, "device / reference units, hyperparameter sets, %s" % gen, t0)
    assert not fails, (len(fails), fails[:30])


def test_constant_y_gives_alpha_exactly_zero(native, ctx):
    """sd = 0 takes the `sd = 1` branch of `k_zstats`: y_s = 0 and alpha = 0 exactly, not merely small."""
    case = G.make_case("lhs", 65, 5, const_y=True)
    _condition(native, ctx, case)
    st = _raw_state(native, ctx)
    assert st["y_std"] == 1.0 and st["y_mean"] == 900.0
    assert not np.any(st["alpha"]) and np.all(np.isfinite(st["L"])) and np.all(np.isfinite(st["R"]))


# ---- b. a small problem in a large, used context --------------------------------------------------------------------
@pytest.mark.parametrize("gen", ("lhs", "twins", "shifted"))
def test_small_problem_in_a_used_large_context_equals_a_fresh_small_one(native, ctx, gen):
    """n = 3, 64, 65, 129 conditioned in the shared context right after the largest case (ld = 384 > NP, tiles of a
    6 x 6 factorisation still in the buffers) and in a fresh context of capacity n: L, R (whole n x n blocks) and
    alpha must be the SAME BITS - nothing may depend on the padding, the leading dimension or stale memory."""
    fails = []
    for n, k in ((129, 33), (65, 5), (64, 5), (3, 1)):
        big = G.make_case("cluster" if gen == "lhs" else "lhs", BIG_N, 33)
        _condition(native, ctx, big)
        case = G.make_case(gen, n, k)
        _condition(native, ctx, case)
        used = _raw_state(native, ctx)
        fresh = native.Context(max_n=n, max_d=k, max_q=16)
        _condition(native, fresh, case)
        own = _raw_state(native, fresh)
        fresh.close()
        for key in ("L", "R", "alpha", "norm_bounds"):
            if not _same_bits(used[key], own[key]):
                fails.append((case.id, key, float(np.nanmax(np.abs(used[key] - own[key])))))
    assert not fails, fails


# ---- c. a defined error (the jitter ladder itself: test_gpu_parity.py::test_not_positive_definite_is_reported) -------
def test_a_column_without_a_range_is_an_error_not_a_model(native):
    """All points agree in one column and no bounds are given: the Normalize range is 0, `k_znorm` produces 0 / 0.
    A NaN distance must stay NaN through the clamps of `k_gram` and fail the first pivot that meets it on every rung:
    PCABO_ERR_NOT_PD, as for the reference (which raises) - not an all-ones K that factors and a model that means
    nothing.  The failure leaves no state behind: gp_state() is a call-order error, and the next conditioning in the
    same context equals a fresh context bit for bit."""
    bad = G.make_case("lhs", 70, 3)
    bad.Z[:, 1] = 0.25
    c = native.Context(max_n=129, max_d=8, max_q=16)
    with pytest.raises(native.PcaboError) as err:
        _condition(native, c, bad)
    assert err.value.code == -2                        # PCABO_ERR_NOT_PD (the pivot is not pinned)
    with pytest.raises(native.PcaboError) as err:
        c.gp_state()
    assert err.value.code == -1                        # PCABO_ERR_ARG
    good = G.make_case("lhs", 129, 5)
    _condition(native, c, good)
    after = _raw_state(native, c)
    c.close()
    fresh = native.Context(max_n=129, max_d=8, max_q=16)
    _condition(native, fresh, good)
    own = _raw_state(native, fresh)
    fresh.close()
    for key in ("L", "R", "alpha"):
        assert _same_bits(after[key], own[key]), key
    assert np.all(np.isfinite(after["alpha"]))
