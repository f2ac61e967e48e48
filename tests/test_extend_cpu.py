"""The reference of pcabo_gp_extend (tests/extend_reference.py) proved on the CPU, and the ABI of the new entry points.

1. Closed form against refit.  The bordering step in np.longdouble, point after point, equals gp_reference's long-double chain on the
   n + p points with the held bounds as user bounds and the held statistics.  Both run at u_x = 2^-64 and both solve with K: the
   tolerance is 16 (n + p) cond_1(K) u_x (the form of test_loo_cpu.py), absolute for the rows of L (entries of order 1), relative to
   the largest entry for the rows of R and for alpha.
2. Units.  A plain fp64 numpy restatement of the step stays within 16 units of the long-double step on the same fp64 R, on every
   input of test_gpu_extend.py (this is the condition that those inputs are fair), and every d2 there is positive.  Its first new
   row of L also stays within 16 of the refit units of the EXACT factor's row.
3. Believer mode on the oracle: the mean of the extended model equals the mean before, and the variance follows the fantasy identity
   of test_posterior_cpu.py for two points taken one after the other.
4. Surface: the symbols are declared in pcabo.h, exported by the built library and bound by pcabo._native (no device needed).
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import extend_reference as ER
import gp_reference as G
import pcabo_oracle as O
from posterior_reference import posterior
from wpca_reference import EXTENDED, f64, hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_extended = pytest.mark.skipif(not EXTENDED, reason="np.longdouble is a plain double here")

REFIT = [(n, p, k, hyper) for n in (2, 17, 64, 65) for p in (1, 3) for k in (1, 5) for hyper in ("default", "rbf")]


def _grow(R, row):
    n = R.shape[0]
    out = np.zeros((n + 1, n + 1), dtype=R.dtype)
    out[:n, :n] = R
    out[n] = row
    return out


def _held_case(n, k, hyper):
    case = G.make_case("lhs", n, k, hyper)
    held = ER.held_of(case)
    case.norm_bounds = held[0]                                   # user bounds = the held ones: the n-point chain reads them too
    return case, held


@needs_extended
@pytest.mark.parametrize("n,p,k,hyper", REFIT, ids=lambda v: str(v))
def test_bordering_equals_the_refit(n, p, k, hyper):
    case, held = _held_case(n, k, hyper)
    kinds = tuple(ER.KINDS[(n + k + j) % 4] for j in range(p))
    Xp, yp = ER.new_points(case, held[0], kinds)
    full = ER.reference_state(case, Xp, yp, held)
    Kinv = full.R.T @ full.R
    cond = float(np.abs(full.K).sum(axis=0).max() * np.abs(Kinv).sum(axis=0).max())
    tol = 16.0 * (n + p) * cond * 2.0 ** -64
    R = G.reference(case).R
    Z = case.Z
    worst = {"L": 0.0, "R": 0.0}
    for i in range(p):
        b = ER.step(R, Xp[i], Z, held[0], case.lengthscale, case.noise, case.kernel)
        m = n + i
        worst["L"] = max(worst["L"], float(np.abs(f64(b.L_row - full.L[m, :m + 1])).max()))
        worst["R"] = max(worst["R"], float(np.abs(f64(b.R_row - full.R[m, :m + 1])).max() / np.abs(f64(full.R[m])).max()))
        R, Z = _grow(R, b.R_row), np.vstack([Z, Xp[i:i + 1]])
    alpha = R.T @ (R @ full.ys)
    worst["alpha"] = float(np.abs(f64(alpha - full.alpha)).max() / np.abs(f64(full.alpha)).max())
    print("  n %d p %d k %d %s %s: cond %.2e, tolerance %.2e, distances %s" % (n, p, k, hyper, kinds, cond, tol, worst))
    assert tol < 1e-9                                            # the comparison is a sharp one in every case
    assert max(worst.values()) <= tol, (worst, tol)


@needs_extended
@pytest.mark.parametrize("n,p,k,hyper,kinds", ER.gpu_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_the_units_hold_for_plain_fp64(n, p, k, hyper, kinds):
    case, held = _held_case(n, k, hyper)
    Xp, yp = ER.new_points(case, held[0], kinds)
    ref = G.reference(case)
    R, Z = f64(ref.R), case.Z
    ys = list((case.y - held[1]) / held[2])
    worst = {"L": 0.0, "R": 0.0, "refit": 0.0}
    for i in range(p):
        b = ER.step(R, Xp[i], Z, held[0], case.lengthscale, case.noise, case.kernel)      # the reference ON the fp64 R
        assert float(b.d2) > 64.0 * b.units.d2, (i, float(b.d2), b.units.d2)              # d2 is positive beyond any rounding
        got = ER.border_f64(R, ER.kernel_vector_f64(Xp[i], Z, held[0], case.lengthscale, case.kernel), 1.0 + case.noise)
        assert got is not None
        worst["L"] = max(worst["L"], ER.ratio(hp(got.L_row) - b.L_row, b.units.L_row))
        worst["R"] = max(worst["R"], ER.ratio(hp(got.R_row) - b.R_row, b.units.R_row))
        if i == 0:                                               # ... and against the exact factor's row of the n + 1 points
            exact = ER.reference_state(case, Xp[:1], yp[:1], held)
            worst["refit"] = ER.ratio(hp(got.L_row) - exact.L[n, :n + 1], ER.row_units_refit(ref, b).L_row)
        R, Z = _grow(R, got.R_row), np.vstack([Z, Xp[i:i + 1]])
        ys.append((yp[i] - held[1]) / held[2])
    ys = np.array(ys)
    alpha_ref, unit = ER.alpha_units(R, ys, 2.0 * G.EPS * np.abs(ys[n:]))
    worst["alpha"] = ER.ratio(hp(R.T @ (R @ ys)) - alpha_ref, unit)
    print("  %s: unit ratios %s" % ((n, p, k, hyper, kinds), worst))
    assert max(worst.values()) <= ER.LIMIT, worst


@needs_extended
def test_a_wrong_bordering_is_caught():
    """The units are tight enough to see what they are for: a pivot that forgets the noise, and a row of R without its sign."""
    case, held = _held_case(17, 5, "default")
    Xp, _ = ER.new_points(case, held[0], ("uniform",))
    R = f64(G.reference(case).R)
    b = ER.step(R, Xp[0], case.Z, held[0], case.lengthscale, case.noise, case.kernel)
    ks = ER.kernel_vector_f64(Xp[0], case.Z, held[0], case.lengthscale, case.kernel)
    good, no_noise = ER.border_f64(R, ks, 1.0 + case.noise), ER.border_f64(R, ks, 1.0)
    assert ER.ratio(hp(good.L_row) - b.L_row, b.units.L_row) <= ER.LIMIT
    assert ER.ratio(hp(no_noise.L_row) - b.L_row, b.units.L_row) > ER.LIMIT
    flipped = good.R_row.copy()
    flipped[:-1] *= -1.0
    assert ER.ratio(hp(flipped) - b.R_row, b.units.R_row) > ER.LIMIT


def test_believer_mode_on_the_oracle():
    rng = np.random.default_rng(77)
    for n, k, kernel in ((12, 2, "matern52"), (40, 5, "rbf")):
        Z, y = rng.uniform(-2.0, 2.0, size=(n, k)), rng.normal(size=n) * 30.0 + 200.0
        gp = O.ExactGP(Z, y, kernel=kernel)
        X = rng.uniform(-2.2, 2.2, size=(17, k))
        Xp = rng.uniform(-2.0, 2.0, size=(2, k))
        before = posterior(gp, X)
        sy = before["y_std"]
        g2 = ER.extended(gp, Z, Xp)
        after = posterior(g2, X)
        assert g2.n == n + 2 and np.array_equal(g2.norm_bounds, gp.norm_bounds)
        assert np.abs(after["mean"] - before["mean"]).max() <= 1e-10 * sy        # a believed value teaches the mean nothing
        # the variance: the fantasy identity, one point after the other, each step from the posterior of the model before it
        probes = np.vstack([X, Xp])
        r0 = posterior(gp, probes)
        want1 = r0["raw_variance"] - r0["covariance"][17] ** 2 / (r0["raw_variance"][17] + gp.noise * sy * sy)
        g1 = ER.extended(gp, Z, Xp[:1])
        r1 = posterior(g1, probes)
        assert np.abs(r1["raw_variance"] - want1).max() <= 1e-11 * sy * sy
        want2 = r1["raw_variance"] - r1["covariance"][18] ** 2 / (r1["raw_variance"][18] + gp.noise * sy * sy)
        r2 = posterior(g2, probes)
        assert np.abs(r2["raw_variance"] - want2).max() <= 1e-11 * sy * sy
        # with values: the new standardised targets are (y - m') / s of the HELD statistics
        yp = np.array([250.0, 120.0])
        g3 = ER.extended(gp, Z, Xp, yp)
        assert np.allclose(g3.y_s.numpy()[n:], (yp - float(gp.y_mean)) / float(gp.y_std), rtol=0, atol=1e-15)
        assert np.array_equal(g3.y_s.numpy()[:n], gp.y_s.numpy())


@needs_extended
def test_the_oracle_model_is_the_extended_precision_one():
    case, held = _held_case(17, 5, "default")
    Xp, yp = ER.new_points(case, held[0], ("uniform", "outside", "near1"))
    gp = O.ExactGP(case.Z, case.y, held[0], lengthscale=case.lengthscale, noise=case.noise)
    X = np.random.default_rng(3).uniform(-3.0, 3.0, size=(17, 5))
    for values in (yp, None):
        want = ER.posterior(ER.reference_state(case, Xp, values, held), X)
        got = posterior(ER.extended(gp, case.Z, Xp, values), X)
        s = held[2]
        assert np.abs(f64(hp(got["mean"]) - want["mean"])).max() <= 1e-9 * s
        assert np.abs(f64(hp(got["covariance"]) - want["covariance"])).max() <= 1e-9 * s * s


def test_the_reference_holds_no_tests():
    assert not [name for name, _ in inspect.getmembers(ER, inspect.isfunction) if name.startswith("test")]


def test_surface(native):
    names = ("pcabo_gp_extend", "pcabo_gp_truncate", "pcabo_gp_extended")
    header = open(os.path.join(ROOT, "include", "pcabo.h")).read()
    lib = ctypes.CDLL(native.lib_path())
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in native.EXPORTS
    assert re.search(r"PCABO_EXTEND_BELIEVER\s*=\s*1\b", header)
    assert native.ABI_VERSION == native.LIB.pcabo_abi_version() == 2
    L = native.LIB
    assert [len(f.argtypes) for f in (L.pcabo_gp_extend, L.pcabo_gp_truncate, L.pcabo_gp_extended)] == [5, 2, 3]
    assert callable(native.Context.gp_extend) and callable(native.Context.gp_truncate)
    assert isinstance(native.Context.n_base, property)
    assert L.pcabo_gp_extend(None, None, None, 1, 0) == -1 and L.pcabo_gp_truncate(None, 0) == -1      # no context: refused, no device
    from Algorithms import PCA_BO, Vanilla_BO
    for cls in (PCA_BO, Vanilla_BO):
        with pytest.raises(RuntimeError):
            with cls(budget=10).fantasy(np.zeros((1, 4))):      # outside a run
                pass
