"""The GP likelihood kernels against an extended-precision reference at edge shapes.

`k_mll_grad<false>`, `k_mll_grad<true>`, `k_mll_finish<>` (csrc/kernels_fit.hip) and `mll_assemble` (csrc/host_side.h)
produce every loss and gradient the GP fits step on.  Here they are judged in the error units of `mll_reference`
(first-order analysis of any fp64 implementation of the sums, starting from the device's own conditioned state;
`test_mll_reference_cpu.py` shows a numpy restatement staying under 4 of each, wrong variants leaving them, the formulas
being the loss's derivative and long double being enough).  The device sums in other orders - MFMA chains, lanes, waves,
tiles - so its constants may differ by small factors: the acceptance limit is 16 in every unit, as in
`test_gpu_gp_edges.py`.  The state the sums are taken from is judged separately by `gp_reference` (b).

One context of capacity 257 x 128 serves every case, large problems first: the leading dimension exceeds the padded
size almost everywhere, the partials buffer holds those of a larger tiling, and every small problem meets the remains of
a larger one.  The batched launches are held bit-equal to these single ones by `test_gpu_batch_fit.py` and
`test_gpu_batch_ard.py`.  Not covered: the second trip of `k_mll_finish`'s tile loop (more than 256 tiles, n > 1408).
"""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import gp_reference as G
import mll_reference as M
from test_gpu_gp_edges import _raw_state, _same_bits

pytestmark = pytest.mark.gpu

LIMIT = 16.0
BIG_N, BIG_D = 257, 128
EPS = G.EPS
LBFGSB_CONV_PG = 40                                    # csrc/lbfgsb.h: the norm of the projected gradient <= pgtol
PGTOL = 1e-5
FIT_S2_MIN, FIT_ARD_RHO_MIN = 1e-4, -40.0 * np.log(2.0)


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=BIG_N, max_d=BIG_D, max_q=16)
    t0 = time.time()
    yield c
    c.close()
    print("\ntest_gpu_mll_edges: %.1f s between context creation and close" % (time.time() - t0))


def _mll(c, form, case, theta):
    return (c.gp_mll_ard if form == "ard" else c.gp_mll)(case.y, theta, Z=case.Z)


def _judge(native, c, form, case, theta):
    """One evaluation on the device, its raw state, the reference at that state and the ratios."""
    r = _mll(c, form, case, theta)
    st = _raw_state(native, c)
    ref = M.reference(st, case.Z, case.y, theta, form == "ard")
    return r, st, ref, (None if ref.skip else M.judge(ref, r["loss"], r["grad"]))


# ---- a. the grid against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("part", M.GRID_PARTS)
@pytest.mark.parametrize("form", ("scalar", "ard"))
def test_grid_against_reference(native, ctx, form, part, capsys):
    """What each part of the grid is there for:

    - n = 2 (the smallest the API takes), 3, 17: one tile, mostly identity padding (`i < n && jn`, the trace over i < n
      only); 63, 64: one row of padding short of a tile, an exact tile; 65: tile (1, 0) with a single live row, 3 tiles;
      128, 129: `mll_tile` decoding t = 0 .. 5; 193: 10 tiles; 257: 15 tiles and the second trip of `k_mll_finish`'s
      `i += 256` loop - at k = 1 and k = 5;
    - k = 1, 3, 4, 5, 8, 9, 12, 33, 64, 65, 128 at n = 65, 129 and (n, k) = (20, 100): KP = k rounded up to 4,
      MLL_ARD_CHUNK = 8 with KP = 4, 8, 12 (half chunks), 36, 68, and KP = 128 = PCABO_MAXD (the width of `s_red`,
      `threadIdx.x <= M`);
    - all four generators at (65, 5) and (129, 33): near and exact duplicates across the tile boundary, columns at
      1e3 +- 5e-3;
    - `pairs` at (129, 33), (65, 5), (17, 3): two clusters 1e-6 wide at -1 and +1 under lengthscales of 0.05 - the far
      pairs vanish from S_c and from its unit, the close ones carry both.  These are the states that hold
      `k_mll_grad<true>`'s DIRECT square (a_ci - a_cj)^2: expanded, it is 1e4 to 1e5 units off here and 6e-4 on the
      generators above (`test_mll_reference_cpu.py::test_units_notice_wrong_variants`).
    Thetas: scalar (e^-5, 0, 0), (1e-4, 0.3, -0.5), (0.05, -0.2, 0.8), (0.3, 0.5, 3), (0.05, 0.3, 20.5) - the last on
    softplus's linear branch; ARD those of `test_gpu_ard.py` (one rho_c = 15, one 25) and one with a rho_c = 20.5.
    Per evaluation: the loss, grad[noise], grad[mean] and grad[rho] (ARD: every grad[rho_c]) within 16 units."""
    t0 = time.time()
    worst, fails, count, skipped = M.Worst(), [], 0, 0
    for gen, n, k in M.grid_part(part):
        case = M.make_case(gen, n, k)
        for theta in M.thetas(form, n, k, gen):
            _, _, ref, j = _judge(native, ctx, form, case, theta)
            if j is None:                              # (only where long double is a plain double)
                skipped += 1
                continue
            count += 1
            cid = M.case_id(case, form, theta)
            worst.add(gen, j, cid)
            fails += [(cid, q, getattr(j, q), j.rho_index) for q in M.QUANTITIES if not getattr(j, q) <= LIMIT]
    with capsys.disabled():
        print("\n" + worst.table("device / reference units, %s, %s (%d evaluations, %d without a reference)"
                                 % (form, part, count, skipped)) + "\n  %.1f s" % (time.time() - t0))
    assert not fails, (len(fails), fails[:30])
    assert count and not (G.EXTENDED and skipped)


# ---- b. the state the sums were taken from ------------------------------------------------------------------------------
def _state_ratios(case, theta, st, K, norm_bounds, lengthscale):
    """`gp_reference.judge` of a raw state conditioned at theta: the case carries theta's lengthscale and noise, the
    reference y_s is shifted by the mean constant."""
    cs = SimpleNamespace(**case.__dict__)
    cs.lengthscale, cs.noise, cs.norm_bounds = lengthscale, float(theta[0]), norm_bounds
    g = G.gram_reference(cs)
    if g.skip:
        pytest.skip(g.skip)
    f = G.factor_reference(g.K, g.ys - G.hp(float(theta[1])), g.u_K, g.u_ys)
    g.__dict__.update({key: val for key, val in f.__dict__.items() if key not in ("K", "n")})
    j = G.judge(g, K, st["L"], st["R"], st["alpha"], case.y, st["y_mean"], st["y_std"], st["norm_bounds"])
    return g, j


def _check_state(j, cid, fails):
    fails += [(cid, q, getattr(j, q)) for q in G.QUANTITIES if not getattr(j, q) <= LIMIT]
    fails += [(cid, flag, False) for flag in G.FLAGS if not getattr(j, flag)]


def _check_mean_constant(native, c, case, theta, st, cid, fails):
    """y_std has the bits of a c = 0 conditioning, y_mean is m + s c to two roundings."""
    c.gp_condition(case.y, Z=case.Z)
    plain = _raw_state(native, c)
    m, s, mc = plain["y_mean"], plain["y_std"], float(theta[1])
    if not _same_bits(st["y_std"], s):
        fails.append((cid, "y_std", st["y_std"], s))
    if not abs(G.hp(st["y_mean"]) - (G.hp(m) + G.hp(s) * G.hp(mc))) <= 2.0 * EPS * (abs(m) + abs(s * mc)):
        fails.append((cid, "y_mean", st["y_mean"], m + s * mc))
    if mc == 0.0 and not _same_bits(st["y_mean"], m):
        fails.append((cid, "y_mean at c = 0", st["y_mean"], m))


@pytest.mark.parametrize("n,k", [(193, 1), (129, 5), (65, 5)])
def test_scalar_state_is_right_including_the_mean_constant(native, ctx, n, k, capsys):
    """The state `gp_mll` leaves at each scalar theta, judged by `gp_reference` (K, the Cholesky, root-inverse and alpha
    residuals, alpha's forward error, diag(R), the bounds; the exact flags), within 16 units."""
    t0 = time.time()
    worst, fails = G.Worst(), []
    case = G.make_case("lhs", n, k)
    for theta in M.thetas("scalar", n, k):
        cid = M.case_id(case, "scalar", theta)
        _mll(ctx, "scalar", case, theta)
        st, K = _raw_state(native, ctx), ctx.gram()
        _, j = _state_ratios(case, theta, st, K, None, float(M.softplus64(theta[2])))
        for q in G.QUANTITIES:
            worst.add("lhs", q, getattr(j, q), cid)
        _check_state(j, cid, fails)
        _check_mean_constant(native, ctx, case, theta, st, cid, fails)
    with capsys.disabled():
        print("\n" + worst.table("state after gp_mll / gp_reference units, n = %d, k = %d" % (n, k)) + "\n  %.1f s" % (time.time() - t0))
    assert not fails, fails


@pytest.mark.parametrize("n,k", [(70, 33), (65, 5)])
def test_ard_state_is_right_including_the_fold(native, ctx, n, k, capsys):
    """The same for `gp_mll_ard`, with the state's folded bounds passed as user bounds at lengthscale 1, and the fold
    against its definition: lo as Normalize gives it, |(hi' - lo) - (hi - lo) l_c| <= 4 eps max(|lo|, |hi'|, hi - lo)
    (the 2^-40 floor of `k_zstats` is not active on these two states and six thetas: test_mll_reference_cpu.py walks them
    with the grid; an active floor would also fail the fold check here)."""
    t0 = time.time()
    worst, fails = G.Worst(), []
    case = G.make_case("lhs", n, k)
    plain = G.gram_reference(case)
    if plain.skip:
        pytest.skip(plain.skip)
    for theta in M.thetas("ard", n, k):
        cid = M.case_id(case, "ard", theta)
        _mll(ctx, "ard", case, theta)
        st, K = _raw_state(native, ctx), ctx.gram()
        _, j = _state_ratios(case, theta, st, K, st["norm_bounds"].copy(), 1.0)
        for q in G.QUANTITIES:
            worst.add("lhs", q, getattr(j, q), cid)
        _check_state(j, cid, fails)
        lo2, hi2 = G.hp(st["norm_bounds"][0]), G.hp(st["norm_bounds"][1])
        rng = plain.hi - plain.lo
        cap = 4.0 * EPS * np.maximum(np.maximum(np.abs(G.f64(plain.lo)), np.abs(st["norm_bounds"][1])), G.f64(rng))
        if not G._ratio(lo2 - plain.lo, plain.u_nb) <= LIMIT:
            fails.append((cid, "folded lo", None))
        if not np.all(np.abs(G.f64((hi2 - lo2) - rng * G.hp(M.softplus64(theta[2:])))) <= cap):
            fails.append((cid, "fold", float(np.max(np.abs(G.f64((hi2 - lo2) - rng * G.hp(M.softplus64(theta[2:]))) / cap)))))
        _check_mean_constant(native, ctx, case, theta, st, cid, fails)
    with capsys.disabled():
        print("\n" + worst.table("state after gp_mll_ard / gp_reference units, n = %d, k = %d" % (n, k)) + "\n  %.1f s" % (time.time() - t0))
    assert not fails, fails


# ---- c. a small problem in a large, used context ------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("scalar", "ard"))
def test_small_problem_in_a_used_large_context_equals_a_fresh_small_one(native, ctx, form):
    """(129, 33), (65, 5), (64, 5), (3, 1) evaluated in the shared context right after the (257, 128) case (ld = 320 > NP,
    the partials of 15 tiles with 1 + 128 sums each still in the buffer) and in a fresh context of capacity (n, k): loss
    and gradient must be the SAME BITS - nothing may depend on the padding, the leading dimension or stale memory."""
    fails = []
    big = G.make_case("lhs", BIG_N, BIG_D)
    for n, k in ((129, 33), (65, 5), (64, 5), (3, 1)):
        case = G.make_case("lhs", n, k)
        for theta in M.thetas(form, n, k)[1:2]:
            _mll(ctx, form, big, M.thetas(form, BIG_N, BIG_D)[1])
            used = _mll(ctx, form, case, theta)
            fresh = native.Context(max_n=n, max_d=k, max_q=16)
            try:
                own = _mll(fresh, form, case, theta)
            finally:
                fresh.close()
            if not (_same_bits(used["loss"], own["loss"]) and _same_bits(used["grad"], own["grad"])):
                fails.append((M.case_id(case, form, theta), used["loss"] - own["loss"], np.abs(used["grad"] - own["grad"]).max()))
    assert not fails, fails


# ---- d. loss and gradient on the fit's own path ---------------------------------------------------------------------------
FIT_STATES = ((2, 65, 5), (6, 40, 3))                  # (seed, n, k) of mll_reference.fit_state


@pytest.mark.parametrize("form", ("scalar", "ard"))
def test_fit_ends_where_the_reference_gradient_agrees(native, ctx, form, capsys):
    """(65, 5) and (40, 3): `gp_fit` / `gp_fit_ard`, then `gp_mll` / `gp_mll_ard` at the returned theta, judged in units;
    the fit's loss is that evaluation's, bit for bit.  Where the fit reports warnflag 0 with the projected-gradient stop,
    the REFERENCE's projected gradient at that theta (bounds: s2 >= 1e-4, ARD rho_c >= ln 2^-40) is at most scipy's pgtol
    of 1e-5 plus 16 gradient units in every component.  Measured on an MI355X: both fits of the (65, 5) state stop on the
    function-reduction test (task 41; the reference's projected gradient there is 6.9e-5 and 2.6e-5), both fits of the
    (40, 3) state on the projected gradient (task 40) - the state is there so that the check runs, and the test says so
    if no fit ends that way any more."""
    checked = 0
    for seed, n, k in FIT_STATES:
        Z, y = M.fit_state(seed, n, k)
        case = SimpleNamespace(Z=Z, y=y, n=n, k=k, id="fit-n%d-k%d" % (n, k))
        fit = (ctx.gp_fit_ard if form == "ard" else ctx.gp_fit)(y, Z=Z)
        theta = np.asarray(fit["theta"], dtype=np.float64)
        r, _, ref, j = _judge(native, ctx, form, case, theta)
        if j is None:
            pytest.skip(ref.skip)
        g = G.f64(np.array(ref.grad, dtype=object))
        lower = np.r_[FIT_S2_MIN, -np.inf, np.full(ref.m, FIT_ARD_RHO_MIN if form == "ard" else -np.inf)]
        pg = np.where(g > 0.0, np.minimum(g, theta - lower), g)
        with capsys.disabled():
            print("\n  %s fit at (%d, %d): %d iterations / %d evaluations, warnflag %d, task %d, loss %.6f; units at the result: "
                  % (form, n, k, fit["iterations"], fit["evaluations"], fit["warnflag"], fit["task"], fit["loss"])
                  + " ".join("%s %.3g" % (q, getattr(j, q)) for q in M.QUANTITIES)
                  + "\n  reference projected gradient: max %.3e (pgtol %.0e, asserted where the task is %d)"
                  % (np.abs(pg).max(), PGTOL, LBFGSB_CONV_PG))
        assert _same_bits(r["loss"], fit["loss"])
        bad = [(q, getattr(j, q)) for q in M.QUANTITIES if not getattr(j, q) <= LIMIT]
        assert not bad, bad
        if fit["warnflag"] == 0 and fit["task"] == LBFGSB_CONV_PG:
            checked += 1
            assert np.all(np.abs(pg) <= PGTOL + LIMIT * ref.u_grad), (n, k, pg, ref.u_grad)
    assert checked, "no fit of FIT_STATES ends on the projected-gradient stop: the pgtol check did not run, choose another state"
