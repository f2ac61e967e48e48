"""The leave-one-out reference (tests/loo_reference.py) proved on the CPU, and the ABI of pcabo_gp_loo / pcabo_batch_gp_loo.

1. The closed form on the extended-precision R and alpha of a case equals the brute-force refit of n - 1 points.  Both run in
   np.longdouble (u_x = 2^-64), and both solve with K: the forward error of either is of the order cond(K) u_x times a modest
   function of n.  The tolerance is 16 n cond_1(K) u_x, cond_1 from the reference's own K and K^-1 = R^T R; it applies to the mean in
   LOO standard deviations, to the variance relatively and to z; lpd = -(log 2 pi + log var + z^2) / 2 gets (1 + |z|) of it.
2. The error units hold (limit 16) for a plain fp64 numpy evaluation of the closed form on fp64 R and alpha.
3. libpcabo.so exports both entry points and pcabo._native binds them (no device needed).
"""
import ctypes
import inspect

import numpy as np
import pytest

import loo_reference as LR
from gp_reference import make_case
from wpca_reference import EXTENDED, f64, hp

pytestmark = pytest.mark.skipif(not EXTENDED, reason="np.longdouble is a plain double here")

CASES = [(gen, n, k, "default", 0.0) for gen in ("lhs", "cluster") for n in (2, 3, 17, 65) for k in (1, 5)]
CASES += [("lhs", 65, 5, "default", 0.3),          # a fitted model's constant mean
          ("lhs", 64, 5, "rbf", 0.0)]              # RBF at lengthscale 3 with noise 1e-4: cond(K) of 1e5 and more


def _case(gen, n, k, hyper, mean_c):
    case = make_case(gen, n, k, hyper)
    case.mean_c = mean_c
    return case


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-n%d-k%d-%s-c%g" % c)
def refs(request):
    case = _case(*request.param)
    full = LR.full_reference(case)
    return case, full, LR.closed_form(full.R, full.alpha, case.y, (full.m, full.s))


def test_closed_form_equals_the_refit(refs):
    case, full, cf = refs
    bf = LR.brute_force(case, full)
    Kinv = full.R.T @ full.R
    cond = float(np.abs(full.K).sum(axis=0).max() * np.abs(Kinv).sum(axis=0).max())
    tol = 16.0 * case.n * cond * 2.0 ** -64
    got = {key: getattr(cf, key) for key in LR.KEYS}
    dist = LR.distances(got, bf)
    zmax = float(np.abs(f64(bf.z)).max())
    print("  %s: cond %.2e, tolerance %.2e, distances %s" % (case.id, cond, tol, dist))
    assert tol < 1e-9                                            # the comparison is a sharp one in every case
    assert dist["mean"] <= tol and dist["variance"] <= tol and dist["z"] <= tol, (dist, tol)
    assert dist["lpd"] <= tol * (1.0 + zmax), (dist, tol)
    assert np.all(f64(bf.variance) > 0.0)
    if case.mean_c:                                             # the constant mean is in m' and nowhere else
        assert abs(float(full.m) - (case.y.mean() + case.y.std(ddof=1) * case.mean_c)) < 1e-9


def test_the_units_hold_for_plain_fp64(refs):
    case, full, _ = refs
    R, alpha, ystats = f64(full.R), f64(full.alpha), (float(full.m), float(full.s))
    cf = LR.closed_form(R, alpha, case.y, ystats)               # the reference ON the rounded inputs
    ratios = LR.unit_ratios(LR.closed_form_f64(R, alpha, case.y, ystats), cf)
    print("  %s: unit ratios %s" % (case.id, ratios))
    assert max(ratios.values()) <= LR.LIMIT, ratios


def test_a_wrong_closed_form_is_caught():
    """The units are tight enough to see what they are for: d summed over the whole column block instead of p >= i (one spurious
    term above the diagonal), and a variance that forgets s^2."""
    case = _case("lhs", 17, 5, "default", 0.0)
    full = LR.full_reference(case)
    R, alpha, ystats = f64(full.R), f64(full.alpha), (float(full.m), float(full.s))
    cf = LR.closed_form(R, alpha, case.y, ystats)
    spoiled = np.tril(R).copy()
    spoiled[0, 1] = 1e-3 * R[1, 1]                              # something above the diagonal
    got = LR.closed_form_f64(spoiled, alpha, case.y, ystats)    # p >= i: it is not read
    assert max(LR.unit_ratios(got, cf).values()) <= LR.LIMIT
    d = (spoiled * spoiled).sum(axis=0)                         # every p: it is
    wrong = dict(got, variance=ystats[1] ** 2 / d)
    assert LR.unit_ratios(wrong, cf)["variance"] > LR.LIMIT
    wrong = dict(got, variance=got["variance"] / ystats[1] ** 2)
    assert LR.unit_ratios(wrong, cf)["variance"] > LR.LIMIT


def test_the_reference_holds_no_tests():
    assert not [name for name, _ in inspect.getmembers(LR, inspect.isfunction) if name.startswith("test")]


def test_library_exports_and_binds_the_loo_entry_points(native):
    lib = ctypes.CDLL(native.lib_path())
    for name in ("pcabo_gp_loo", "pcabo_batch_gp_loo"):
        assert hasattr(lib, name), name
        assert name in native.EXPORTS
    assert len(native.LIB.pcabo_gp_loo.argtypes) == 6 and len(native.LIB.pcabo_batch_gp_loo.argtypes) == 7
    assert callable(native.Context.gp_loo) and callable(native.Batch.gp_loo)
    from Algorithms import PCA_BO, Vanilla_BO
    for cls in (PCA_BO, Vanilla_BO):
        with pytest.raises(RuntimeError):
            cls(budget=10).loo()                                # outside a run
