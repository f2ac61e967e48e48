"""The extended-precision reference of the GP conditioning chain and its error units, proved without a GPU.

`test_gpu_gp_edges.py` holds the HIP kernels to 16 of the units of `gp_reference`.  That is only worth something if
an independent fp64 implementation of the documented chain - `gp_reference.restate`: norms + dot product for the
distance, np.linalg.cholesky, scipy's solve_triangular, two mat-vecs - stays well inside them on the same grid
(limit 4, the margin of the wPCA proof), and if wrong variants of it leave them (more than 16).  The same file
asserts what the device tests rely on without checking it themselves: every grid case is positive definite with a
wide margin at the first rung of the jitter ladder, every jitter input at the second.
"""
import numpy as np
import pytest

import gp_reference as G

LIMIT = 4.0
DEVICE_LIMIT = 16.0
EPS = G.EPS
NUMERIC = ("K", "chol", "rinv", "alpha_res", "alpha_fw", "diag", "bounds")


def _judge_restatement(case, ref, worst, bad):
    res = G.restate(case)
    j = G.judge(ref, res.K, res.L, res.R, res.alpha, case.y, res.y_mean, res.y_std, res.norm_bounds)
    for q in NUMERIC:
        v = getattr(j, q)
        worst.add(case.gen, q, v, case.id)
        if not v <= LIMIT:
            bad.append((case.id, q, v))
    for flag in G.FLAGS:
        if not getattr(j, flag):
            bad.append((case.id, flag, False))
    # rung 0 is decisively positive definite: the noise alone is far above what rounding can move an eigenvalue by
    margin = case.noise / (case.n * EPS * np.linalg.norm(res.K, 2))
    if not margin >= 1e3:
        bad.append((case.id, "noise / (n eps ||K||)", margin))
    return j


@pytest.mark.parametrize("part", G.GRID_PARTS)
@pytest.mark.parametrize("gen", G.GENERATORS)
def test_restatement_within_units_on_grid(gen, part, capsys):
    """Every (n, k) of the device grid with the default hyperparameters: K, the Cholesky, root-inverse and alpha
    residuals, the forward error of alpha, diag(R) diag(L) and the Normalize bounds of the fp64 restatement, each
    <= 4 units; noise >= 1e3 n eps ||K||_2."""
    worst, bad, skipped = G.Worst(), [], 0
    sizes = G.grid_part(part)
    for n, k in sizes:
        case = G.make_case(gen, n, k)
        ref = G.reference(case)
        if ref.skip:
            skipped += 1
            continue
        _judge_restatement(case, ref, worst, bad)
    with capsys.disabled():
        print("\n" + worst.table("fp64 restatement / reference units, %s, %s (%d cases, %d skipped)"
                                 % (gen, part, len(sizes), skipped)))
    assert not bad, bad[:20]
    assert skipped < len(sizes) and not (G.EXTENDED and skipped)


@pytest.mark.parametrize("gen", G.GENERATORS)
def test_restatement_within_units_on_hyperparameter_sets(gen, capsys):
    """Short lengthscale with little noise, the ill-conditioned RBF set and user bounds wider than the data."""
    worst, bad = G.Worst(), []
    for n, k, hyper in G.hyper_sizes():
        case = G.make_case(gen, n, k, hyper)
        ref = G.reference(case)
        if ref.skip:
            pytest.skip(ref.skip)
        _judge_restatement(case, ref, worst, bad)
    with capsys.disabled():
        print("\n" + worst.table("fp64 restatement / reference units, hyperparameter sets, %s" % gen))
    assert not bad, bad[:20]


def test_grid_is_the_issue_grid():
    sizes = G.grid_sizes()
    assert len(sizes) == len(set(sizes)) == 14 * 3 + 2 * 10 - 2 * 3
    assert {n for n, _ in sizes} == set(G.GRID_N) and {k for _, k in sizes} == set(G.GRID_K)
    assert [n for n, _ in sizes] == sorted((n for n, _ in sizes), reverse=True)
    assert sorted(sum((G.grid_part(p) for p in G.GRID_PARTS), [])) == sorted(sizes)
    assert {-(-n // 64) for n, _ in sizes} == {1, 2, 3, 4, 5, 6}
    assert len(G.hyper_sizes()) == 3 * 2 * 3
    twins = G.make_case("twins", 193, 5).Z
    assert np.array_equal(twins[0], twins[65]) and np.array_equal(twins[126], twins[191])
    cl = G.make_case("cluster", 129, 5).Z
    rng = cl.max(axis=0) - cl.min(axis=0)
    mid = (cl[-96:].max(axis=0) + cl[-96:].min(axis=0)) / 2
    assert (np.abs(cl[-96:] - mid) <= 1e-3 * rng).all() and 96 * 4 >= 3 * 128
    sh = G.make_case("shifted", 65, 8).Z
    assert np.allclose(sh / sh.mean(axis=0), 1.0, atol=5.1e-6) and sh.mean(axis=0).max() / sh.mean(axis=0).min() > 1e11


def test_constant_y_gives_alpha_exactly_zero():
    """sd = 0 takes the `sd = 1` branch; y_s and alpha are exactly 0 in the reference and in the restatement."""
    case = G.make_case("lhs", 65, 5, const_y=True)
    ref = G.reference(case)
    if ref.skip:
        pytest.skip(ref.skip)
    res = G.restate(case)
    assert float(ref.sd) == 1.0 and res.y_std == 1.0
    assert not np.any(G.f64(ref.alpha)) and not np.any(res.alpha)


def _worst_ratio(case, ref, **wrong):
    res = G.restate(case, **wrong)
    j = G.judge(ref, res.K, res.L, res.R, res.alpha, case.y, res.y_mean, res.y_std, res.norm_bounds)
    return {q: getattr(j, q) for q in NUMERIC}


def test_units_notice_wrong_variants():
    """The units are not vacuous: four wrong variants of the restatement, each above the DEVICE's limit of 16 in the
    quantity it damages, on a grid case where the right one is below 4 everywhere."""
    case = G.make_case("lhs", 193, 5)
    ref = G.reference(case)
    if ref.skip:
        pytest.skip(ref.skip)
    assert max(_worst_ratio(case, ref).values()) <= LIMIT
    blocked = G.restate(case)
    blocked_L = G.blocked_cholesky(blocked.K)                      # (the blocked form itself is a right one)
    assert G._ratio(G.hp(blocked_L) @ G.hp(blocked_L).T - G.hp(blocked.K), ref.u_C) <= LIMIT
    # one panel product dropped, for the last block row only
    # (k = 33: K is far enough from singular for the damaged factorisation to stay positive definite)
    wide = G.make_case("lhs", 193, 33)
    r = _worst_ratio(wide, G.reference(wide), drop=(3, 2, 0))
    assert r["chol"] > DEVICE_LIMIT and r["alpha_res"] > DEVICE_LIMIT, r
    # j < i instead of j <= i in t = R y_s
    r = _worst_ratio(case, ref, matvec_strict=True)
    assert r["alpha_res"] > DEVICE_LIMIT and r["alpha_fw"] > DEVICE_LIMIT and r["chol"] <= LIMIT, r
    # the 5/3 of the Matern map rounded to float
    r = _worst_ratio(case, ref, coef53=np.float32(5.0 / 3.0))
    assert r["K"] > DEVICE_LIMIT, r
    # the same on the short-lengthscale set, where the unit is at its widest
    short = G.make_case("lhs", 65, 1, "short")
    r = _worst_ratio(short, G.reference(short), coef53=np.float32(5.0 / 3.0))
    assert r["K"] > DEVICE_LIMIT, r
    # an explicit inverse that lost one element
    res = G.restate(case)
    R = res.R.copy()
    R[130, 3] = 0.0
    j = G.judge(ref, res.K, res.L, R, res.alpha, case.y, res.y_mean, res.y_std, res.norm_bounds)
    assert j.rinv > DEVICE_LIMIT


@pytest.mark.parametrize("case", G.jitter_cases(), ids=lambda c: c.id)
def test_jitter_inputs_are_positive_definite_at_rung_one(case):
    """With noise = 0 these K are singular up to rounding: rung 0 of the ladder may go either way.  Rung 1 must not:
    lambda_min(K + 1e-8 I) >= 1e3 n eps ||K||_2 for the restatement's K, and the restatement factored at rung 1
    stays within 4 units of the reference factorisation of its own K + 1e-8 I."""
    res = G.restate(case, jitter=1e-8)
    lam = np.linalg.eigvalsh(res.K_factored)
    bound = 1e3 * case.n * EPS * np.linalg.norm(res.K, 2)
    assert lam[0] >= bound, (lam[0], bound)
    assert np.linalg.eigvalsh(res.K)[0] < bound                    # and it is rung 1 that makes it so
    if not G.EXTENDED and case.n > G.MP_MAX_N:
        pytest.skip("no extended-precision factorisation of n = %d here" % case.n)
    ys = (G.hp(case.y) - G.hp(res.y_mean)) / G.hp(res.y_std)
    fref = G.factor_reference(G.hp(res.K_factored), ys)
    j = G.judge_factor(fref, res.K, res.L, res.R, res.alpha, case.y, res.y_mean, res.y_std, K_factored=res.K_factored)
    for q in ("chol", "rinv", "alpha_res", "alpha_fw", "diag"):
        assert getattr(j, q) <= LIMIT, (q, getattr(j, q))
    assert j.upper_zero and j.diag_positive


def test_a_column_without_a_range_is_an_error_in_the_reference():
    """All points agree in one column and no bounds are given: zn = 0 / 0, the NaN reaches the Cholesky and the
    reference raises - there is no model to return."""
    case = G.make_case("lhs", 20, 3)
    case.Z[:, 1] = 0.25
    if not G.EXTENDED:
        pytest.skip("the NaN path is exercised with np.longdouble only")
    with pytest.raises(G.NotPositiveDefinite):
        G.reference(case)
    with pytest.raises((np.linalg.LinAlgError, ValueError)):       # (LAPACK's factorisation or scipy's check of its input)
        G.restate(case)
