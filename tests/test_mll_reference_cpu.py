"""The extended-precision reference of the GP fit's loss and gradient and its error units, proved without a GPU.

`test_gpu_mll_edges.py` holds `k_mll_grad<>`, `k_mll_finish<>` and `mll_assemble` to 16 of the units of
`mll_reference`.  That is worth something only if (a) an independent fp64 restatement of the documented sums stays
well inside them on a grid of the device's shapes (limit 4, the margin of the other reference proofs), (b) wrong
variants of it leave them (more than 16) on a named state, (c) the on-state formulas are the derivative of the loss
computed with no state at all, and (d) long double is enough to stand for "exact" (40-digit mpmath agrees to 1e-3
units).  The states come from a host conditioning (`mll_reference.host_state`).
"""
import math

import mpmath
import numpy as np
import pytest

import gp_reference as G
import mll_reference as M

LIMIT = 4.0
DEVICE_LIMIT = 16.0
FD_CAP = 1e-8
MP_CAP = 1e-3


def _inv_softplus(ls):
    return math.log(math.expm1(ls))


def _cpu_theta(form, case, ls, s2):
    if form == "scalar":
        return np.array([s2, M.CPU_MEAN_C, _inv_softplus(ls)])
    rng = np.random.default_rng([case.n, case.k, 77])
    return np.r_[s2, M.CPU_MEAN_C, [_inv_softplus(ls * f) for f in rng.uniform(0.5, 2.0, size=case.k)]]


def _both(case, theta, ard, **wrong):
    """Ratios of the restatement's sums and of its loss and gradient on a host state."""
    st = M.host_state(case, theta, ard)
    ref = M.reference(st, case.Z, case.y, theta, ard)
    if ref.skip:
        pytest.skip(ref.skip)
    slope = wrong.pop("sigmoid_above_threshold", False)
    h = M.restate_sums(st, case.Z, case.y, theta, ard, **wrong)
    loss, grad = M.restate_assemble(h, case.n, theta, ard, sigmoid_above_threshold=slope)
    return ref, M.judge_sums(ref, h), M.judge(ref, loss, grad)


# ---- a. the restatement within the units ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("scalar", "ard"))
@pytest.mark.parametrize("gen", G.GENERATORS)
def test_restatement_within_units_on_grid(gen, form, capsys):
    """n = 3, 64, 65, 129 x k = 1, 5, 33, 128 x (l, s2) = (ln 2, e^-5), (0.2, 1e-4), (3, 0.05) with c = 0.3 (ARD: the
    lengthscales spread over [l / 2, 2 l]): h0 .. h4, S (every S_c), the loss and every gradient component of the fp64
    restatement, each <= 4 units."""
    ws, wj, rel = M.Worst(M.SUMS), M.Worst(), []
    for n in M.CPU_N:
        for k in M.CPU_K:
            case = G.make_case(gen, n, k)
            for ls, s2 in M.CPU_HYPERS:
                theta = _cpu_theta(form, case, ls, s2)
                ref, js, j = _both(case, theta, form == "ard")
                cid = M.case_id(case, form, theta)
                ws.add("l=%.2g" % ls, js, cid)
                wj.add("l=%.2g" % ls, j, cid)
                rel.append(float(ref.u_S[0] / abs(G.f64(ref.S[0]))))
    with capsys.disabled():
        print("\n" + ws.table("fp64 restatement / units of the sums, %s, %s" % (form, gen)))
        print(wj.table("fp64 restatement / units of loss and gradient, %s, %s" % (form, gen)))
        print("  uS / |S| (first S): %.1e .. %.1e" % (min(rel), max(rel)))
    bad = ws.failures(LIMIT) + wj.failures(LIMIT)
    assert not bad, bad


# ---- b. wrong variants leave the units --------------------------------------------------------------------------------
LIN = np.array(M.SCALAR_THETAS[4])                                       # (0.05, 0.3, 20.5)
MID = np.array(M.SCALAR_THETAS[2])                                       # (0.05, -0.2, 0.8)
PAIRS = "the theta of the `pairs` states"                                # (mll_reference.pairs_theta)


def _ard_theta(case, s2=0.05):
    return _cpu_theta("ard", case, G.LENGTHSCALE, s2)


VARIANTS = [
    # (name, form, (gen, n, k), theta or None (ARD: seeded), wrong keywords, the quantity that must leave)
    ("trace over the padded rows", "scalar", ("lhs", 3, 1), MID, {"trace_padded": True}, "h4"),
    ("trace over the padded rows", "scalar", ("lhs", 65, 5), MID, {"trace_padded": True}, "h4"),
    ("tile (1, 0) counted once", "scalar", ("lhs", 65, 5), MID, {"tile10_once": True}, "S"),
    ("tile (1, 0) counted once", "ard", ("lhs", 65, 5), None, {"tile10_once": True}, "S"),
    ("first row of block I left out of Kinv", "scalar", ("lhs", 65, 5), MID, {"skip_first_row": True}, "h4"),
    ("first row of block I left out of Kinv", "scalar", ("lhs", 129, 5), MID, {"skip_first_row": True}, "S"),
    ("5/3 in float32", "scalar", ("lhs", 17, 3), MID, {"coef53": np.float32(5.0 / 3.0)}, "S"),
    ("5/3 in float32", "ard", ("lhs", 17, 3), None, {"coef53": np.float32(5.0 / 3.0)}, "S"),
    ("sigmoid slope at rho = 20.5", "scalar", ("lhs", 3, 1), LIN, {"sigmoid_above_threshold": True}, "g_rho"),
    ("sigmoid slope at rho = 20.5", "scalar", ("lhs", 17, 3), LIN, {"sigmoid_above_threshold": True}, "g_rho"),
    ("sigmoid slope at rho = 20.5", "scalar", ("lhs", 65, 5), LIN, {"sigmoid_above_threshold": True}, "g_rho"),
    ("square expanded", "ard", ("pairs", 17, 3), PAIRS, {"expanded_square": True}, "S"),
    ("square expanded", "ard", ("pairs", 65, 5), PAIRS, {"expanded_square": True}, "S"),
    ("square expanded", "ard", ("pairs", 129, 33), PAIRS, {"expanded_square": True}, "S"),
    ("square expanded", "ard", ("cluster", 65, 5), None, {"expanded_square": True}, "S (listed)"),
    ("square expanded", "ard", ("shifted", 65, 5), None, {"expanded_square": True}, "S (listed)"),
    ("inputs c >= 8 dropped", "ard", ("lhs", 65, 9), None, {"drop_second_chunk": True}, "S"),
    ("S_c in slot c + 1", "ard", ("lhs", 65, 5), None, {"shift_slots": True}, "S"),
]


def test_units_notice_wrong_variants(capsys):
    """Each wrong variant of the restatement is beyond the DEVICE's limit of 16 in the quantity it damages, on the
    state named beside it, where the right restatement is below 4 everywhere.

    The ARD square expanded as a_i^2 + a_j^2 - 2 a_i a_j is asserted on the `pairs` states (two clusters 1e-6 wide under
    lengthscales of 0.05: the far pairs vanish from S_c and from its unit, the close ones carry both; these states are in
    the device grid).  On `cluster` and `shifted` (65, 5) the same variant is only LISTED with its margin, 2e-4 and 6e-4
    units: there the far pairs set uS_c through the error the norm + GEMM distance is allowed, which has the size of the
    expansion's, so those two states do not pin the direct square on the device either."""
    lines, bad = [], []
    for name, form, (gen, n, k), theta, wrong, q in VARIANTS:
        case = M.make_case(gen, n, k)
        theta = _ard_theta(case) if theta is None else M.pairs_theta(form, k) if theta is PAIRS else theta
        _, js, j = _both(case, theta, form == "ard")
        right = max([getattr(js, s) for s in M.SUMS] + [getattr(j, s) for s in M.QUANTITIES])
        _, ws, wj = _both(case, theta, form == "ard", **dict(wrong))
        v = getattr(wj if q.startswith("g_") else ws, q.split()[0])
        lines.append("  %-40s %-7s %-22s %-12s %10.3g units (right variant: worst %.2g)" % (name, form, case.id, q, v, right))
        if not ((v > DEVICE_LIMIT or q.endswith("(listed)")) and right <= LIMIT):
            bad.append((name, form, case.id, q, v, right))
    with capsys.disabled():
        print("\nwrong variants, units of the damaged quantity:\n" + "\n".join(lines))
    assert not bad, bad


def test_the_fold_floor_is_not_active_on_the_ard_states():
    """`k_zstats` holds a folded range at 2^-40 of max(|lo|, range); no theta of either test file is near it, so
    `hi' - lo = (hi - lo) l_c` is the model every ARD state is judged against (host_state asserts it per state): the
    whole device grid and the (70, 33) state of the device's fold check."""
    shapes = [c for part in M.GRID_PARTS for c in M.grid_part(part)] + [("lhs", 70, 33)]
    for gen, n, k in shapes:
        lo, hi = M.data_bounds(M.make_case(gen, n, k).Z)
        for theta in M.thetas("ard", n, k, gen):
            assert not M.fold(lo, hi, M.softplus64(theta[2:]))[1], (gen, n, k)
    lo, hi = np.array([1e3]), np.array([1e3 + 1e-2])
    assert M.fold(lo, hi, np.array([1e-8]))[1] and not M.fold(lo, hi, np.array([1e-5]))[1]


def test_device_grid_holds_every_shape_it_is_there_for():
    assert M.grid_part("pairs") == [("pairs", 129, 33), ("pairs", 65, 5), ("pairs", 17, 3)]
    pz = M.pairs_case(65, 5).Z
    assert np.all(np.abs(np.abs(pz) - 1.0) <= M.PAIRS_WIDTH) and np.all(pz[0::2] < 0) and np.all(pz[1::2] > 0)
    assert [n for _, n, _ in M.grid_part("n-k1")] == [257, 193, 129, 128, 65, 64, 63, 17, 3, 2]
    assert sorted(k for _, _, k in M.grid_part("k-n129")) == [1, 3, 4, 5, 8, 9, 12, 33, 64, 65, 128]
    assert M.grid_part("k-n65")[-1] == ("lhs", 20, 100) and len(M.grid_part("k-n65")) == 12
    assert len(M.grid_part("generators")) == 8
    assert {(k + 3) // 4 * 4 for k in M.GRID_K} == {4, 8, 12, 36, 64, 68, 128}
    for n, k in ((65, 5), (129, 128)):
        th = M.ard_thetas(n, k)
        assert len(th) == 6 and 15.0 in th[3] and 25.0 in th[4] and 20.5 in th[5]
    assert [t[2] for t in M.SCALAR_THETAS] == [0.0, -0.5, 0.8, 3.0, 20.5]


# ---- c. the on-state gradient is the derivative of the loss --------------------------------------------------------------
@pytest.mark.parametrize("form", ("scalar", "ard"))
@pytest.mark.parametrize("n,k", [(24, 2), (40, 5), (65, 3)])
def test_gradient_is_the_derivative_of_the_loss_from_scratch(n, k, form, capsys):
    """Richardson-extrapolated central differences (step 1e-4, relative for s2) of `loss_from_scratch` - Normalize,
    Gram, Cholesky in long double, no state - against the on-state formulas at a long-double-conditioned state:
    within 1e-8 of each component's term scale (the extrapolation's own error is O(h^4)).  One theta above softplus's
    threshold in each form: the derivative there is 1."""
    if not G.EXTENDED:
        pytest.skip("the difference quotients need np.longdouble")
    ard = form == "ard"
    case = G.make_case("lhs", n, k)
    if ard:
        rng = np.random.default_rng([n, k, 5])
        rho = rng.uniform(-0.5, 1.5, size=k)
        lin = rho.copy()
        lin[k - 1] = 20.5
        ths = [np.r_[0.05, 0.3, rho], np.r_[0.02, -0.1, lin]]
    else:
        ths = [MID, LIN]
    worst = 0.0
    for theta in ths:
        ref = M.reference(M.scratch_state(case.Z, case.y, theta, ard), case.Z, case.y, theta, ard)
        assert abs(float(ref.loss - M.loss_from_scratch(case.Z, case.y, theta, ard))) <= 1e-15 * max(1.0, abs(float(ref.loss)))
        x = [G.hp(float(t)) for t in theta]
        for j in range(len(theta)):
            step = G.hp(1e-4) * (x[0] if j == 0 else 1)
            fd = M.richardson(lambda th: M.loss_from_scratch(case.Z, case.y, th, ard), x, j, step)
            err = abs(float(fd - ref.grad[j])) / ref.t_grad[j]
            worst = max(worst, err)
            assert err <= FD_CAP, (theta, j, float(fd), float(ref.grad[j]), ref.t_grad[j])
    with capsys.disabled():
        print("\n  (n, k) = (%d, %d), %s: gradient against extrapolated differences, worst %.1e of the term scale (cap %.0e)"
              % (n, k, form, worst, FD_CAP))


# ---- d. long double against 40 digits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("scalar", "ard"))
def test_long_double_agrees_with_mpmath(form, capsys):
    """At n <= 40 every sum, the loss and every gradient component of the long-double reference agree with the same
    formulas evaluated with 40 digits to 1e-3 units."""
    ard = form == "ard"
    worst = 0.0
    for gen, n, k in (("lhs", 3, 1), ("lhs", 17, 3), ("cluster", 40, 5), ("twins", 33, 4)):
        case = G.make_case(gen, n, k)
        for theta in M.thetas(form, n, k)[1:]:
            st = M.host_state(case, theta, ard)
            ref = M.reference(st, case.Z, case.y, theta, ard)
            if ref.skip:
                pytest.skip(ref.skip)
            with mpmath.workdps(40):
                X = M.mp_arith(40)
                ex = M.sums(st, case.Z, case.y, theta, ard, arith=X)
                pairs = [(ref.h[i], ex.h[i], ref.u_h[i]) for i in range(5)]
                pairs += [(ref.S[i], ex.S[i], ref.u_S[i]) for i in range(ref.m)]
                pairs += [(ref.loss, ex.loss, ref.u_loss)] + [(ref.grad[i], ex.grad[i], ref.u_grad[i]) for i in range(2 + ref.m)]
                for mine, exact, unit in pairs:
                    top = float(mine)                      # a long double is the exact sum of two doubles
                    err = abs(float(mpmath.mpf(top) + mpmath.mpf(float(mine - top)) - exact))
                    assert unit > 0.0
                    worst = max(worst, err / unit)
                    assert err <= MP_CAP * unit, (case.id, theta, float(exact), err, unit)
    with capsys.disabled():
        print("\n  long double against 40-digit mpmath, %s: worst %.1e units (cap %.0e)" % (form, worst, MP_CAP))
