"""The extended-precision wPCA reference and its error units, proved on the sklearn path (no GPU).

`test_gpu_wpca_edges.py` judges the HIP kernels by `wpca_reference`: limit 16 in every unit.  That is only
worth something if an independent fp64 implementation - numpy + sklearn/LAPACK, `oracle.weighted_pca(...,
use_sklearn=True)` - sits well inside the same units on the same grid.  Measured worst ratios of that path:
residual 0.44, orthogonality 1.33, evr 0.27, data_mean 0.33, pca_mean 2.8 (`shifted`, d = 64, n = 1050); the
assertion is <= 4 for every quantity, so a change of the reference machinery is noticed.

The grid's cases must also decide the number of components exactly: no cumulative rho / sum(rho) within 1e-9
of the 0.95 threshold (then `k` can be asserted, not compared loosely).
"""
import numpy as np
import pytest

import pcabo_oracle as O
import wpca_reference as R

LIMIT = 4.0
MARGIN = 1e-9


def _cases(gen):
    return [c for c in R.grid_cases() if c[0] == gen]


@pytest.mark.parametrize("gen", R.GENERATORS)
def test_sklearn_path_within_units_on_grid(gen, capsys):
    """Whole grid (d = 1 .. 128 incl. odd d, d % 16 != 0, 63/64/65; n = 2 .. 1050 incl. n <= d) for one generator:
    residual, orthogonality, evr, sign rule and both means of the sklearn path in the reference's units."""
    worst, bad, near, skipped = R.Worst(), [], [], 0
    for g, d, n in _cases(gen):
        case = R.make_case(g, d, n)
        ref = R.reference(case.X, case.ranks, case.noise)
        if ref.skip:
            skipped += 1
            continue
        res = O.weighted_pca(case.X, None, False, 0.95, 0, noise=case.noise, use_sklearn=True, ranks=case.ranks)
        assert res.components.shape == (min(n, d), d)
        inv = R.judge(ref, res.data_mean, res.pca_mean, res.components, res.evr)
        for q in R.QUANTITIES:
            v = getattr(inv, q)
            worst.add(g, q, v, case.id)
            if not v <= LIMIT:
                bad.append((case.id, q, v))
        for flag in ("finite", "evr_monotone", "sign_ok", "dead_ok"):
            if not getattr(inv, flag):
                bad.append((case.id, flag, False))
        # selection condition, on the reference's eigenvalues and on sklearn's Rayleigh quotients
        if min(R.cumulative_margin(ref.rho), R.cumulative_margin(inv.rho)) <= MARGIN:
            near.append(case.id)
        k_ref = O.select_components(ref.rho / ref.rho.sum(), 0.95, 0)
        if res.k != k_ref:
            bad.append((case.id, "k", (res.k, k_ref)))
    with capsys.disabled():
        print("\n" + worst.table("sklearn path / reference units, %s (%d cases, %d skipped)"
                                 % (gen, len(_cases(gen)), skipped)))
    assert not near, "cumulative variance within 1e-9 of the threshold (change the seed): %s" % near
    assert not bad, bad[:20]
    if not R.EXTENDED:
        assert skipped < len(_cases(gen))


def test_grid_is_the_issue_grid():
    cases = R.grid_cases()
    assert len(cases) == len(set(cases)) == 4 * 181                # 186 (d, n) combinations, five of them repeats
    assert all(n >= 2 for _, _, n in cases)
    assert {d for _, d, _ in cases} == set(R.GRID_D)


def test_units_notice_a_wrong_result():
    """The units are tight enough to see the failures the device test is there for: a dropped row, a leaked pad
    value, a sweep stopped at 1e-8 - each is far above 16 units."""
    case = R.make_case("cluster", 17, 31)
    ref = R.reference(case.X, case.ranks, case.noise)
    if ref.skip:
        pytest.skip(ref.skip)
    res = O.weighted_pca(case.X, None, False, 0.95, 0, noise=case.noise, use_sklearn=True, ranks=case.ranks)
    good = R.judge(ref, res.data_mean, res.pca_mean, res.components, res.evr)
    assert max(getattr(good, q) for q in R.QUANTITIES) <= LIMIT
    # a covariance that lost its last row
    drop = O.weighted_pca(case.X[:-1], None, False, 0.95, 0, noise=case.noise[:-1], use_sklearn=True,
                          ranks=R.stable_ranks(case.f[:-1]))
    assert R.judge(ref, res.data_mean, res.pca_mean, drop.components, drop.evr).residual > 1e6
    # two components rotated into each other by 1e-8 (a Jacobi sweep that stopped early)
    comps = res.components.copy()
    comps[0], comps[1] = comps[0] + 1e-8 * comps[1], comps[1] - 1e-8 * comps[0]
    assert R.judge(ref, res.data_mean, res.pca_mean, comps, res.evr).residual > 1e4
    # a mean off by one part in 1e12
    assert R.judge(ref, res.data_mean * (1 + 1e-12), res.pca_mean, res.components, res.evr).data_mean > 1e2


def test_stable_ranks_ties_by_index():
    f = np.array([1000.0, 0.0, -0.0, 1000.0, -1.0, 0.0])
    assert R.stable_ranks(f).tolist() == [5, 2, 3, 6, 1, 4]
    assert R.stable_ranks(f, maximize=True).tolist() == [1, 3, 4, 2, 6, 5]
