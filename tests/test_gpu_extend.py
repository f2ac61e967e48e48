"""Appending points to a conditioned GP on the MI355X and taking them back (pcabo_gp_extend / pcabo_gp_truncate: k_ext_ks,
k_ext_append, k_ext_truncate of kernels_ext.hip; Context.gp_extend / gp_truncate, PCA_BO.fantasy, Vanilla_BO.fantasy) against
tests/extend_reference.py.

Comparisons, kept apart:
  kernel arithmetic  rows n .. of L and R as gp_state() hands them out against the long-double bordering step applied to the DEVICE's
                     own R, bounds and statistics with the extended-precision kernel vector (extend_reference.step), 16 units; rows
                     < n byte-equal to before; alpha against the long-double R^T (R y_s) on the device's own R, 16 units.
  end to end         gp_posterior (mean and covariance at 17 probes), gp_loo and acq_eval (log-EI, value and gradient, q = 3 and
                     q = 70, and the value-only GEMM route at q = 70) of the extended context against a fresh long-double
                     factorisation of the n + p points with the device's bounds and statistics held (extend_reference.reference_state).
                     The yardstick of a case is the distance of the plain numpy / LAPACK fp64 restatement (restated_state) from the
                     same reference; the device may be 32 x that away - the margin of test_gpu_loo.py, for the same reason: the
                     explicit root inverse - or, where the yardstick is smaller, 16 of the first-order units, per entry
                     (acq_reference's for the posterior and the acquisition, loo_reference's for the LOO vectors).  Measured: the
                     largest device / yardstick ratio is 32.1 (z of the LOO at 129 -> 130, k = 33, the new point an exact copy of
                     training point 0: d2 = 2 s2 there, and v = R ks through the explicit inverse loses against LAPACK's
                     substitution, which happens to land within 6e-15); it lies inside 16 of its units (0.1 of them).
  round trip         after gp_truncate() gp_state, acq_eval, gp_posterior with covariance, gp_loo and optimize_acqf (resident path
                     and PCABO_OPT_GROUP_ACQ) return the bytes recorded before the extend, at every shape.
The shapes are extend_reference.gpu_cases(): the padding written at 64 -> 65 and in the middle of 127 -> 130, with a throw-away
200-point conditioning in front of the 64 -> 65 cases so that the capacity buffers hold stale data where the padding goes.  The
padded block has no reader of its own: it is seen through the posterior, the acquisition and the LOO of the extended context, whose
kernels read all NP rows.
"""
import numpy as np
import pytest
import torch

import acq_reference as AR
import extend_reference as ER
import gp_reference as G
import loo_reference as LR
from pcabo.bbob import BBOBProblem
from wpca_reference import EPS, f64, hp

pytestmark = pytest.mark.gpu

ALLOWED, UNITS = 32.0, 16.0
ERR_ARG, NOT_PD = -1, -2
RATIOS = {}                                                      # (case) -> what the end-to-end comparison measured, for the report


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=256, max_d=65, max_q=128)
    yield c
    c.close()


def _kernel(native, case):
    return native.KERNEL_RBF if case.kernel == "rbf" else native.KERNEL_MATERN52


def _condition(native, ctx, case, **kw):
    ctx.gp_condition(case.y, Z=case.Z, norm_bounds=case.norm_bounds, lengthscale=case.lengthscale, noise=case.noise,
                     kernel=_kernel(native, case), **kw)


def _probes(case, q, seed):
    lo, hi = case.Z.min(axis=0), case.Z.max(axis=0)
    return np.random.default_rng([seed, case.n, case.k]).uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), size=(q, case.k))


def _best(case):
    return float(np.float32(np.median(case.y)))                  # (the library rounds the incumbent to float32 as botorch does)


def _state_bytes(st):
    return [st[key].tobytes() for key in ("L", "R", "alpha", "norm_bounds")] + [np.float64(st["y_mean"]).tobytes(),
                                                                                np.float64(st["y_std"]).tobytes()]


def _snapshot(native, ctx, case, optimise=True):
    """The bytes of everything the round trip promises."""
    best = _best(case)
    out = _state_bytes(ctx.gp_state())
    for q in (3, 70):
        out += [a.tobytes() for a in ctx.acq_eval(_probes(case, q, 1), best)]
    out.append(ctx.acq_eval(_probes(case, 70, 1), best, grad=False).tobytes())
    post = ctx.gp_posterior(_probes(case, 17, 2), covariance=True)
    out += [post[key].tobytes() for key in ("mean", "variance", "covariance")]
    loo = ctx.gp_loo()
    out += [np.asarray(loo[key]).tobytes() for key in LR.KEYS + ("lpd_sum",)]
    if optimise:
        box = ctx.acq_bounds()
        ics = np.random.default_rng([3, case.n, case.k]).uniform(box[0], box[1], size=(6, case.k))
        for group in (0, 1):
            ctx.set_option(native.OPT_GROUP_ACQ, group)
            try:
                cand, vals, info, _ = ctx.optimize_acqf(ics, box, best, batch_limit=3)
            finally:
                ctx.set_option(native.OPT_GROUP_ACQ, 0)
            out += [cand.tobytes(), vals.tobytes(), info.tobytes()]
    return out


def _within(dev_err, yard_err, unit):
    """Every error of the device within 32 x the restatement's largest, or within 16 of its own first-order units."""
    dev_err, unit = np.abs(f64(dev_err)), np.asarray(unit, dtype=np.float64)
    yard = float(np.abs(f64(yard_err)).max())
    ok = bool(np.all(np.isfinite(dev_err)) and np.all(dev_err <= np.maximum(ALLOWED * yard, UNITS * unit)))
    return ok, float(dev_err.max()), yard


def _kernel_arithmetic(case, st0, st1, Xp, yp, what):
    """Rows n .. of the device's L and R in the units of the long-double step on the device's own R; alpha likewise."""
    n, p = case.n, Xp.shape[0]
    assert st1["L"][:n, :n].tobytes() == st0["L"].tobytes() and st1["R"][:n, :n].tobytes() == st0["R"].tobytes(), what
    assert np.all(np.triu(st1["L"], 1) == 0.0) and np.all(np.triu(st1["R"], 1) == 0.0)
    Z, worst = case.Z, {"L": 0.0, "R": 0.0}
    for i in range(p):
        m = n + i
        b = ER.step(st1["R"][:m, :m], Xp[i], Z, st0["norm_bounds"], case.lengthscale, case.noise, case.kernel)
        worst["L"] = max(worst["L"], ER.ratio(hp(st1["L"][m, :m + 1]) - b.L_row, b.units.L_row))
        worst["R"] = max(worst["R"], ER.ratio(hp(st1["R"][m, :m + 1]) - b.R_row, b.units.R_row))
        Z = np.vstack([Z, Xp[i:i + 1]])
    ys = (hp(np.concatenate([case.y, yp])) - hp(st0["y_mean"])) / hp(st0["y_std"])
    alpha_ref, unit = ER.alpha_units(st1["R"], ys, 2.0 * EPS * np.abs(f64(ys[n:])))
    worst["alpha"] = ER.ratio(hp(st1["alpha"]) - alpha_ref, unit)
    print("  %s: kernel arithmetic, units %s" % (what, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= ER.LIMIT, (what, worst)


def _end_to_end(ctx, case, st0, Xp, yp, what):
    held = (st0["norm_bounds"], float(st0["y_mean"]), float(st0["y_std"]))
    ref, res = ER.reference_state(case, Xp, yp, held), ER.restated_state(case, Xp, yp, held)
    ast, s, best = ER.acq_state(ref.case), held[2], _best(case)
    seen, bad = {}, []

    def judge(name, dev_err, yard_err, unit):
        ok, d, y = _within(dev_err, yard_err, unit)
        seen[name] = (d, y, d / y if y > 0.0 else float("inf") if d > 0.0 else 0.0)
        if not ok:
            bad.append(name)

    # the posterior at 17 probes: mean in units of s, covariance in units of s^2
    X = _probes(case, 17, 2)
    lin = AR.linear(ast, ref.gs, X)
    dev, rp, sp = ctx.gp_posterior(X, covariance=True), ER.posterior(ref, X), ER.posterior(res, X)
    u_mean = lin.dmus + 2.0 * EPS * (abs(held[1]) / s + np.abs(f64(lin.mus)))
    u_var = lin.dvv + EPS * (1.0 + 3.0 * np.abs(f64(1 - lin.vv)))
    judge("mean", (hp(dev["mean"]) - rp["mean"]) / s, (hp(sp["mean"]) - rp["mean"]) / s, u_mean)
    judge("cov", (hp(dev["covariance"]) - rp["covariance"]) / (s * s), (hp(sp["covariance"]) - rp["covariance"]) / (s * s),
          np.maximum(u_var[:, None], u_var[None, :]))
    # the leave-one-out vectors of the n + p points
    y_ext = ref.case.y
    cf = LR.closed_form(ref.R, ref.alpha, y_ext, (held[1], s))
    loo = ctx.gp_loo()
    assert all(loo[key].shape == (case.n + Xp.shape[0],) for key in LR.KEYS)
    rl, un, sd = LR.closed_form_f64(res.R, res.alpha, y_ext, (held[1], s)), LR.units(cf), f64(np.sqrt(cf.variance))
    floors = {"mean": un["mean"] / sd, "variance": un["variance"] / f64(cf.variance), "z": un["z"], "lpd": un["lpd"]}

    def loo_errors(got):                                         # the measures of loo_reference.distances, per point
        return {"mean": (hp(got["mean"]) - cf.mean) / hp(sd), "variance": hp(got["variance"]) / cf.variance - 1,
                "z": hp(got["z"]) - cf.z, "lpd": hp(got["lpd"]) - cf.lpd}

    dl, yl = loo_errors(loo), loo_errors(rl)
    for key in LR.KEYS:
        judge("loo_" + key, dl[key], yl[key], floors[key])
    # log-EI: per-query kernels (q = 3), the route of q = 70 with gradients, and the value-only GEMM scoring
    for q in (3, 70):
        Xq = _probes(case, q, 1)
        sc = AR.scalars(AR.linear(ast, ref.gs, Xq), best, 0, AR.LOG_EI)
        rv, rg = AR.restate(ast, res.gs, Xq, best, 0, AR.LOG_EI)
        v, g = ctx.acq_eval(Xq, best)
        judge("logei%d" % q, hp(v) - sc.value, hp(rv) - sc.value, sc.u_value)
        judge("grad%d" % q, hp(g) - sc.grad, hp(rg) - sc.grad, sc.u_grad)
        if q == 70:
            judge("score70", hp(ctx.acq_eval(Xq, best, grad=False)) - sc.value, hp(rv) - sc.value, sc.u_value)
    RATIOS[what] = seen
    print("  %s: device / yardstick %s" % (what, " ".join("%s %.1e/%.1e=%.2f" % ((k,) + v) for k, v in seen.items())))
    assert not bad, (what, bad, seen)


# ---- every shape: kernel arithmetic, end to end, round trip ------------------------------------------------------------------
@pytest.mark.parametrize("n,p,k,hyper,kinds", ER.gpu_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_extend_and_take_back(native, ctx, n, p, k, hyper, kinds):
    case = G.make_case("lhs", n, k, hyper)
    what = "%d->%d k%d %s %s" % (n, n + p, k, hyper, "/".join(kinds))
    if n == 64:                                                  # dirty capacity: stale rows and columns where the padding goes
        _condition(native, ctx, G.make_case("lhs", 200, k, hyper))
    _condition(native, ctx, case)
    assert ctx.n_base == n
    before, st0 = _snapshot(native, ctx, case), ctx.gp_state()
    Xp, yp = ER.new_points(case, st0["norm_bounds"], kinds)
    assert ctx.gp_extend(Xp, yp) == n + p == ctx.n and ctx.n_base == n
    st1 = ctx.gp_state()
    _kernel_arithmetic(case, st0, st1, Xp, yp, what)
    _end_to_end(ctx, case, st0, Xp, yp, what)
    again = ctx.gp_state()                                       # the queries changed nothing
    assert _state_bytes(again) == _state_bytes(st1)
    assert ctx.gp_truncate() == n == ctx.n
    assert _snapshot(native, ctx, case) == before, what
    # the same call on the same state gives the same bytes
    ctx.gp_extend(Xp, yp)
    assert _state_bytes(ctx.gp_state()) == _state_bytes(st1)
    ctx.gp_truncate()


@pytest.mark.parametrize("n", [63, 64, 127])
def test_extend_extend_truncate_to_the_first(native, ctx, n):
    """extend, extend, truncate(n + 1): the state after the first extend alone - across a change of NP in either call."""
    case = G.make_case("lhs", n, 5)
    _condition(native, ctx, case)
    before = _snapshot(native, ctx, case)
    Xp, yp = ER.new_points(case, ctx.gp_state()["norm_bounds"], ("uniform", "near1", "outside"))
    ctx.gp_extend(Xp[:1], yp[:1])
    first = _snapshot(native, ctx, case)
    ctx.gp_extend(Xp[1:], yp[1:])
    assert ctx.n == n + 3 and ctx.n_base == n
    assert ctx.gp_truncate(n + 1) == n + 1
    assert _snapshot(native, ctx, case) == first
    ctx.gp_truncate()
    assert _snapshot(native, ctx, case) == before
    ctx.gp_extend(Xp, yp)                                        # three points in one call or in two: the same bytes
    one_call = _state_bytes(ctx.gp_state())
    ctx.gp_truncate()
    ctx.gp_extend(Xp[:1], yp[:1])
    ctx.gp_extend(Xp[1:], yp[1:])
    assert _state_bytes(ctx.gp_state()) == one_call
    _condition(native, ctx, case)                                # a new conditioning starts over
    assert ctx.n == n == ctx.n_base and _snapshot(native, ctx, case) == before


# ---- believer mode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hyper", [(64, "default"), (65, "rbf")])
def test_believer_mode(native, ctx, n, hyper):
    """The mean does not move (within the end-to-end tolerance of the two states), the variance follows the fantasy identity on
    gp_posterior's own covariance: after one point x,  var'(a) = var(a) - cov(a, x)^2 / (var(x) + s2 s^2).  Each of the five
    covariance entries of that statement carries at most 16 units, and |cov(a, x)| <= var(x) + s2 s^2: 16 * 5 units."""
    case = G.make_case("lhs", n, 5, hyper)
    _condition(native, ctx, case)
    st0 = ctx.gp_state()
    held = (st0["norm_bounds"], float(st0["y_mean"]), float(st0["y_std"]))
    s = held[2]
    Xp, _ = ER.new_points(case, held[0], ("uniform", "outside"))
    X = np.vstack([_probes(case, 17, 2), Xp[:1]])
    p0 = ctx.gp_posterior(X, covariance=True)
    ctx.gp_extend(Xp[:1])
    p1 = ctx.gp_posterior(X, covariance=True)
    c0 = p0["covariance"]
    want = np.diag(c0) - c0[:, 17] ** 2 / (c0[17, 17] + case.noise * s * s)
    lin = AR.linear(ER.acq_state(case), ER.reference_state(case, Xp[:0], None, held).gs, X)
    unit = float((lin.dvv + EPS * (1.0 + 3.0 * np.abs(f64(1 - lin.vv)))).max())
    err = np.abs(np.diag(p1["covariance"]) - want).max() / (s * s)
    print("  believer %d %s: fantasy identity %.2e, allowed %.2e" % (n, hyper, err, 5 * UNITS * unit))
    assert err <= 5 * UNITS * unit
    ctx.gp_extend(Xp[1:])                                        # the second point sees the first
    assert ctx.n == n + 2
    p2 = ctx.gp_posterior(X, covariance=True)
    # the mean: both states against their long-double references, the yardsticks of both, 32 x the larger (or 16 units)
    ref0, res0 = ER.reference_state(case, Xp[:0], None, held), ER.restated_state(case, Xp[:0], None, held)
    ref2, res2 = ER.reference_state(case, Xp, None, held), ER.restated_state(case, Xp, None, held)
    yard = max(np.abs(f64(hp(ER.posterior(res0, X)["mean"]) - ER.posterior(ref0, X)["mean"])).max(),
               np.abs(f64(hp(ER.posterior(res2, X)["mean"]) - ER.posterior(ref2, X)["mean"])).max()) / s
    u_mean = float((lin.dmus + 2.0 * EPS * (abs(held[1]) / s + np.abs(f64(lin.mus)))).max())
    moved = np.abs(p2["mean"] - p0["mean"]).max() / s
    print("  believer %d %s: mean moved %.2e, yardstick %.2e, unit %.2e" % (n, hyper, moved, yard, u_mean))
    assert moved <= 2.0 * max(ALLOWED * yard, UNITS * u_mean)
    assert np.abs(f64(hp(p2["mean"]) - ER.posterior(ref2, X)["mean"])).max() / s <= max(ALLOWED * yard, UNITS * u_mean)
    assert np.all(np.diag(p2["covariance"]) <= np.diag(p1["covariance"]) + 5 * UNITS * unit * s * s)
    # y is not read in believer mode: the raw entry point with yp = NULL and the flag
    ctx.gp_truncate()
    Zp = np.ascontiguousarray(Xp)
    ctx._chk(native.LIB.pcabo_gp_extend(ctx._h, native._ptr(Zp), None, 2, 1))
    ctx.n = n + 2
    assert ctx.gp_posterior(X, covariance=True)["mean"].tobytes() == p2["mean"].tobytes()
    ctx.gp_truncate()


def test_device_pointer_mode(native, ctx):
    case = G.make_case("lhs", 65, 5)
    _condition(native, ctx, case)
    Xp, yp = ER.new_points(case, ctx.gp_state()["norm_bounds"], ("uniform", "copy0"))
    ctx.gp_extend(Xp, yp)
    host = _state_bytes(ctx.gp_state())
    ctx.gp_truncate()
    dX, dy = torch.from_numpy(Xp).cuda(), torch.from_numpy(yp).cuda()
    torch.cuda.synchronize()
    assert native.LIB.pcabo_set_pointer_mode(ctx._h, native.PTR_DEVICE) == 0
    try:
        rc = native.LIB.pcabo_gp_extend(ctx._h, native.C.c_void_p(dX.data_ptr()), native.C.c_void_p(dy.data_ptr()), 2, 0)
    finally:
        assert native.LIB.pcabo_set_pointer_mode(ctx._h, native.PTR_HOST) == 0
    assert rc == 0
    ctx.n = 67
    assert _state_bytes(ctx.gp_state()) == host
    ctx.gp_truncate()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _refused(native, call, code=ERR_ARG):
    with pytest.raises(native.PcaboError) as e:
        call()
    assert e.value.code == code


def test_refusals_leave_the_state_alone(native):
    case = G.make_case("lhs", 64, 3)
    c = native.Context(max_n=70, max_d=3, max_q=32)
    L, p = native.LIB, native._ptr
    good = np.ascontiguousarray(case.Z[:7] + 0.01)
    vals = np.full(7, 900.0)
    try:
        c.k = 3
        _refused(native, lambda: c.gp_extend(good[:1], vals[:1]))                             # never conditioned
        _refused(native, lambda: c.gp_truncate(0))
        _condition(native, c, case)
        state = _state_bytes(c.gp_state())

        def unchanged():
            assert c.n_base == 64 and c.n == 64 and _state_bytes(c.gp_state()) == state

        raw = lambda Z, y, n, flags: c._chk(L.pcabo_gp_extend(c._h, p(Z), p(y), n, flags))       # noqa: E731
        _refused(native, lambda: raw(good, vals, 0, 0))                                       # p < 1
        _refused(native, lambda: raw(good, vals, -3, 0))
        unchanged()
        _refused(native, lambda: raw(good, vals, 7, 0))                                       # n + p = max_n + 1
        unchanged()
        _refused(native, lambda: raw(None, vals, 1, 0))                                       # Zp NULL
        _refused(native, lambda: raw(good, None, 1, 0))                                       # yp NULL without the believer flag
        _refused(native, lambda: raw(good, vals, 1, 2))                                       # unknown flag bits
        _refused(native, lambda: raw(good, vals, 1, 1 | 4))
        unchanged()
        for bad_value in (np.nan, np.inf, -np.inf):
            Zb, yb = good.copy(), vals.copy()
            Zb[2, 1] = bad_value
            _refused(native, lambda: raw(Zb, vals, 3, 0))                                     # a coordinate that is not finite
            yb[1] = bad_value
            _refused(native, lambda: raw(good, yb, 2, 0))                                     # a value that is not finite
        unchanged()
        _refused(native, lambda: c.gp_truncate(63))                                           # n0 outside n_base .. n
        _refused(native, lambda: c.gp_truncate(65))
        unchanged()
        assert c.gp_extend(good[:6], vals[:6]) == 70                                          # n + p = max_n is accepted
        _refused(native, lambda: raw(good, vals, 1, 0))                                       # ... and nothing fits behind it
        _refused(native, lambda: c.gp_truncate(71))
        assert c.gp_truncate(64) == 64
        unchanged()
        _condition(native, c, case, wait=False)
        _refused(native, lambda: c.gp_extend(good[:1], vals[:1]))                             # between _begin and its _end
        _refused(native, lambda: c.gp_truncate(64))
        c.gp_wait()
        unchanged()
    finally:
        c.close()


def test_not_positive_definite_is_taken_back(native):
    """A pivot that fails, without anything being provoked on the device.  The issue's input - noise 1e-300 and an exact duplicate
    of a training point - leaves d2 = 1 - |v|^2 at rounding size, of either sign (tests/test_extend_cpu.py's restatement gives it in
    fp64; the device sums in another order): whichever way it falls there, the call is all or nothing.  The nearest input whose d2
    fails in EVERY fp64 arithmetic is a finite point so far away that its normalised squared distance overflows: ks is NaN, d2 is
    NaN, the call returns PCABO_ERR_NOT_PD and the state bytes are those of before - also as the third point of a call."""
    case = G.make_case("lhs", 63, 3)
    case.noise = 1e-300
    c = native.Context(max_n=80, max_d=3, max_q=32)
    try:
        _condition(native, c, case)
        state = _state_bytes(c.gp_state())
        dup, far = case.Z[:1].copy(), np.full((1, 3), 1e200)
        fine = np.ascontiguousarray(case.Z[5:7] + 0.37)
        try:                                                     # the duplicate: rounding decides, the contract holds either way
            c.gp_extend(dup, [900.0])
            c.gp_truncate()
        except native.PcaboError as e:
            assert e.code == NOT_PD
        assert c.n == 63 and c.n_base == 63 and _state_bytes(c.gp_state()) == state
        _refused(native, lambda: c.gp_extend(far, [900.0]), NOT_PD)
        assert "positive definite" in c._err()
        assert c.n == 63 and _state_bytes(c.gp_state()) == state
        _refused(native, lambda: c.gp_extend(np.vstack([fine, far]), [900.0, 800.0, 700.0]), NOT_PD)      # the third of three, NP grows before it
        assert c.n == 63 and c.n_base == 63 and _state_bytes(c.gp_state()) == state
        _refused(native, lambda: c.gp_extend(np.vstack([far, fine])), NOT_PD)                 # believer mode, the first of three
        assert _state_bytes(c.gp_state()) == state
        assert c.gp_extend(fine, [900.0, 800.0]) == 65                                       # and the context goes on
        c.gp_truncate()
        assert _state_bytes(c.gp_state()) == state
    finally:
        c.close()


# ---- the optimiser classes: a visit inside a run changes nothing ------------------------------------------------------------------
class _Stop(Exception):
    pass


def _visiting(base):
    class Visiting(base):
        def optimize_acqf_and_get_observation(self):
            new = super().optimize_acqf_and_get_observation()
            n = len(self.f_evals)
            X = np.random.default_rng(n).uniform(-5.0, 5.0, size=(4, 5))
            before = self.posterior(X)
            with self.fantasy(X, [1.0, 2.0, 3.0, 4.0]) as same:
                assert same is self
                inside, loo = self.posterior(X), self.loo()
            with self.fantasy(X[:2]):                            # believer mode
                held = self.posterior(X)
            try:
                with self.fantasy(X):
                    raise _Stop()                                # the body raises: the points are still taken back
            except _Stop:
                pass
            after = self.posterior(X)
            self.seen.append((n, before, inside, loo, held, after))
            return new
    return Visiting


@pytest.mark.parametrize("name,kw", [("PCA_BO", {}), ("PCA_BO", {"acq_kernel": "group"}), ("Vanilla_BO", {})],
                         ids=["PCA_BO", "PCA_BO-group", "Vanilla_BO"])
def test_fantasy_inside_a_run(name, kw):
    import Algorithms
    base = getattr(Algorithms, name)
    runs = []
    for cls in (base, _visiting(base)):
        opt = cls(budget=12, n_DoE=8, random_seed=15051, **kw, **({"fantasy_points": 4} if cls is not base else {}))
        opt.seen = []
        opt(problem=BBOBProblem(15, 0, 5), dim=5, bounds=np.array([-5.0, 5.0]))
        runs.append(opt)
    plain, probed = runs
    assert np.array(plain.x_evals).tobytes() == np.array(probed.x_evals).tobytes()
    assert np.array(plain.f_evals, dtype=np.float64).tobytes() == np.array(probed.f_evals, dtype=np.float64).tobytes()
    assert len(probed.seen) == 4
    for n, before, inside, loo, held, after in probed.seen:
        assert all(loo[key].shape == (n + 4,) for key in LR.KEYS)
        assert all(after[key].tobytes() == before[key].tobytes() for key in before)
        assert np.all(inside["variance"] <= before["variance"] * (1.0 + 1e-9))      # four more observations
        assert np.abs(inside["mean"] - before["mean"]).max() > 0.0
        assert np.allclose(held["mean"][:2], before["mean"][:2], rtol=1e-6, atol=1e-6 * np.abs(before["mean"]).max())
    with pytest.raises(RuntimeError):
        with probed.fantasy(np.zeros((1, 5))):                   # the run is over
            pass
