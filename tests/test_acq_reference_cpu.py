"""The extended-precision reference of log-EI and PI and its error units, proved without a GPU.

`test_gpu_acq_edges.py` holds every evaluation path of the HIP kernels to 16 of the units of `acq_reference`.  That is
only worth something if an independent fp64 implementation of the chain - `acq_reference.restate`: numpy, the direct
distance, `R @ ks`, the three branches of `log_ei_helper` through scipy's erfcx / erfc / log1p - stays well inside them
(limit 4, the margin of the wPCA and GP proofs) on conditioned states of `gp_reference.restate`, and if wrong variants
of it leave them (more than 16, on the small states more than 1600).  The same file asserts what the device test
relies on without checking it itself: the hand-placed queries, the branches the incumbents reach, no variance within
rounding of the 1e-10 floor.  The four stress states (n385k65, n449k83, n1025, n1473) are proved like the others; the
wrong variants must be seen on the first of them, and the arithmetic that puts each code form at its state is asserted.
"""
import numpy as np
import pytest

import acq_reference as A

LIMIT = 4.0
DEVICE_LIMIT = 16.0
PROVED = A.SMALL_STATES + ["C"] + A.STRESS_STATES     # every state with n <= 130, n = 449, and the stress states
WRONG_ON = A.SMALL_STATES + ["C", "n385k65"]          # where the wrong variants must be seen: + the first stress state
_REFS = {}


def _refs(name):
    """label -> (acq, maximize, best_f, reference) of a state on its restated conditioning, computed once."""
    if name not in _REFS:
        _, _, lin = A.prepared(name)
        _REFS[name] = {label: (acq, mx, best, A.scalars(lin, best, mx, acq)) for label, acq, mx, best in A.cases(lin)}
    return _REFS[name]


@pytest.mark.parametrize("name", PROVED)
def test_restatement_within_units(name, capsys):
    """Values and gradients of the fp64 restatement at all 130 queries of every scalar of the state: <= 4 units."""
    st, gs, _ = A.prepared(name)
    worst, bad = {}, []
    for label, (acq, mx, best, ref) in _refs(name).items():
        v, g = A.restate(st, gs, st.X, best, mx, acq)
        rv, rg = A.judge(ref, v, g)
        worst[label] = (rv, rg)
        if not (rv <= LIMIT and rg <= LIMIT):
            bad.append((label, rv, rg))
    with capsys.disabled():
        print("\n[fp64 restatement / reference units, state %s (n=%d k=%d %s)] worst value %.3g gradient %.3g"
              % (name, st.n, st.k, st.kernel, max(w[0] for w in worst.values()), max(w[1] for w in worst.values())))
    assert not bad, bad


def _helper_grid():
    """u from 38 down to -1e10 across every branch, 50 points within 1e-6 of -1 and 40 around the -1e6 seam."""
    rng = np.random.default_rng(77)
    up = np.concatenate([np.linspace(38.0, -0.999, 400), -1.0 + 10.0 ** rng.uniform(-12, -0.5, 20)])
    mid = -(10.0 ** np.concatenate([np.linspace(0.0, 5.999, 480), rng.uniform(0.0, 6.0, 20)]))
    tail = -(10.0 ** np.linspace(6.0, 10.0, 200))
    seam1 = -1.0 + np.concatenate([rng.uniform(-1e-6, 1e-6, 46), [0.0, 2.0 ** -53, -2.0 ** -52, 1e-6]])
    seam6 = -1e6 + np.concatenate([rng.uniform(-1.0, 1.0, 30), rng.uniform(-1e-6, 1e-6, 6), [0.0, 2.0 ** -33, -2.0 ** -33, 1e-9]])
    return np.concatenate([up, mid, tail, seam1, seam6])


def test_helper_restatement_within_units_and_derivative_error_table(capsys):
    """`log_ei_helper` alone, as scipy evaluates it, against the exact h = log(phi + u Phi) and h' = Phi / ei: within 4
    of u_h and u_dh at every grid point (u is exact here: each point is judged in the unit of its own branch).  Prints
    the TRUE relative error of h' by decade of |u|: the cancellation of w'(u) in botorch's middle branch, which the
    units carry and the kernels share."""
    u = _helper_grid()
    assert len(u) == 1210 and (u > -1.0).sum() > 400 and ((u <= -1.0) & (u > -1e6)).sum() > 500 and (u <= -1e6).sum() > 200
    assert (np.abs(u + 1.0) <= 1e-6).sum() >= 50 and (np.abs(u + 1e6) <= 1.0).sum() >= 40
    h, dh = A.helper_restated(u)
    worst, table = [0.0, 0.0], {}
    for ui, hi, di in zip(u, h, dh):
        eh, ed, _, u_h, u_dh = A.helper_units(float(ui))
        rh, rd = abs(float(A.MP.mpf(hi) - eh)) / u_h, abs(float(A.MP.mpf(di) - ed)) / u_dh
        worst = [max(worst[0], rh), max(worst[1], rd)]
        if ui <= -1.0:
            dec = int(np.floor(np.log10(-ui)))
            rel, unit = abs(float((A.MP.mpf(di) - ed) / ed)), u_dh / abs(float(ed))
            table[dec] = (max(table.get(dec, (0, 0))[0], rel), max(table.get(dec, (0, 0))[1], unit))
    with capsys.disabled():
        print("\n[log_ei_helper restated / units over %d points] worst h %.3g, h' %.3g" % (len(u), worst[0], worst[1]))
        print("  |u| in            true relative error of h'     u_dh / |h'|")
        for dec in sorted(table):
            print("  [1e%d, 1e%d)       %10.2e                 %10.2e" % (dec, dec + 1, table[dec][0], table[dec][1]))
    assert worst[0] <= LIMIT and worst[1] <= LIMIT, worst


@pytest.mark.parametrize("variant", list(A.WRONG))
def test_units_notice_wrong_variant(variant, capsys):
    """The units are not vacuous: each wrong variant of the restatement leaves the DEVICE's limit of 16 in at least one
    case of every state it applies to, and on the states up to n = 70 by more than 100 times - with one deviation from
    that second condition, decided by the reference and not by a state's name.

    The float32 5/3 scales every gradient by 1 + rho exactly, rho = 2.4e-8, so it stands rho |g| / u_grad above the
    reference and no higher (`acq_reference._float32_strength`, reference quantities only).  The test asserts that the
    restatement with the variant is seen at that strength (at least half of it: the right restatement's own error is
    below 1), above 16 everywhere, and 100-fold on the states up to n = 70 WHERE THAT STRENGTH EXCEEDS 1600.  It does on
    all of them but n64 (112 units): 64 points on a LINE (k = 1) at the default lengthscale give alpha entries up to
    308 with alternating signs, A_c = sum_j alpha_j cf_j d_j cancels ten-thousandfold (sum of |terms| / |A_c| = 9872 at
    the worst query), and the gradient's unit is 1e6 eps of the gradient.  Three quarters of dA_c there are
    (n + 4) eps of the sum of the absolute terms - the worst case of ANY summation order, which cannot be cut for an
    implementation whose order is not assumed - and the remaining quarter (the first-order terms of d, sq and cf under
    the same cancellation) caps what dropping that term could gain at a factor of four.  No unit can hold this state to
    1600.  Every other variant is seen on n64 4000-fold and more."""
    kw, what, applies = A.WRONG[variant][:3]
    strength = A.WRONG[variant][3] if len(A.WRONG[variant]) > 3 else None
    seen, bad = [], []
    for name in WRONG_ON:
        st, gs, _ = A.prepared(name)
        worst = predicted = None
        for label, (acq, mx, best, ref) in _refs(name).items():
            if not applies(st, label, ref):
                continue
            v, g = A.restate(st, gs, st.X, best, mx, acq, **kw)
            rv, rg = A.judge(ref, v, g)
            r = {"value": rv, "grad": rg, "any": max(rv, rg)}[what]
            worst = r if worst is None else max(worst, r)
            if strength is not None:
                predicted = max(predicted or 0.0, strength(ref))
        if worst is None:
            continue
        seen.append("%s %.3g" % (name, worst) + ("" if predicted is None else " (of %.3g)" % predicted))
        hundredfold = st.n <= 70 and (predicted is None or predicted > 100.0 * DEVICE_LIMIT)
        if not worst > DEVICE_LIMIT * (100.0 if hundredfold else 1.0):
            bad.append((name, worst))
        if predicted is not None and not worst >= 0.5 * predicted:
            bad.append((name, worst, "below the strength the reference predicts", predicted))
    with capsys.disabled():
        print("\n[%s: worst %s ratio per state] %s" % (variant, what, "; ".join(seen)))
    assert seen and not bad, bad


@pytest.mark.parametrize("name", list(A.STATES))
def test_case_inputs_satisfy_the_conditions_of_the_device_test(name):
    """Two training points, a training point + 1e-9 and a duplicate within the first five queries; every incumbent puts
    the first 32 queries on the branch it is meant for; states E / mixed hold clamped / both kinds of variances; no
    variance lies within 32 dvar of the floor (such a query was redrawn, none skipped)."""
    st, _, lin = A.prepared(name)
    assert st.X.shape == (A.Q, st.k) and min(A.PREFIXES) > max(A.FIXED_QUERIES)
    assert len(A.cases(lin)) == 16
    assert A.check_conditions(name, st, lin) == []
    assert len(st.redrawn) <= 8 and not set(st.redrawn) & set(A.FIXED_QUERIES)


@pytest.mark.parametrize("name", A.HIGH_K_STATES)
def test_high_k_stress_states_see_their_training_points(name, capsys):
    """Why the two high-k states carry a lengthscale of their own: the median |v|^2 over the queries is at least 0.01,
    so the gradient parts through R (w = R^T v, B_c) stand above rounding and a wrong one leaves the unit.  At the
    default ln 2 it is 2e-3 or less."""
    st, _, lin = A.prepared(name)
    vv = A.f64(lin.vv)
    with capsys.disabled():
        print("\n[state %s (n=%d k=%d), lengthscale %g] |v|^2 median %.3g, range %.3g .. %.3g"
              % (name, st.n, st.k, st.lengthscale, np.median(vv), vv.min(), vv.max()))
    assert st.lengthscale > A.LENGTHSCALE and np.median(vv) >= 0.01


def test_stress_states_reach_the_forms_their_comments_name():
    """The arithmetic of the comments beside the stress states, from the constants of the library's sources as the
    comments quote them: ACQ_SLAB32_NP = 448, PCABO_QA_MAX = 416, k_acq_group up to NP = 1280 with ceil(NP / 256)
    columns per thread and launch_acq_group's LDS formula (GQ = 5, GT_LD = 17)."""
    shape = {name: (64 * -(-A.STATES[name][0] // 64), A.STATES[name][1]) for name in A.STRESS_STATES}
    assert shape == {"n385k65": (448, 65), "n449k83": (512, 83), "n1025": (1088, 5), "n1473": (1536, 2)}
    assert set(A.STRESS_STATES) <= set(A.STATES) and set(A.STRESS_STATES) <= set(A.POSTERIOR_STATES)

    def group_lds(NP, k):
        ke = (k + 1) & ~1
        return 8 * (5 * max(NP, 2 * ke) + 4 * 64 * 17 + 64 * 8 + 5 * 64 + 2 * 5 + 4 + 2 * 5 + 5 * ke + 8)

    assert [group_lds(512, 83), group_lds(512, 82)] == [65568, 65488] and group_lds(512, 82) <= 65536 < group_lds(512, 83)
    assert group_lds(448, 65) <= 65536 and -(-448 // 256) == 2 and -(-1088 // 256) == 5 and 1088 <= 1280 < 1536
    assert len(range(0, 65, 32)) == 3 and len(range(0, 65, 64)) == 2 and len(range(0, 83, 64)) == 2
    assert [5 * 65, 6 * 65, 5 * 83, 6 * 83] == [325, 390, 415, 498] and 415 <= 416 < 498 and 32 * 65 > 416
    assert [1088 // 32, 1536 // 32, 1088 // 64, 1536 // 64] == [34, 48, 17, 24] and 34 > 18
    assert all(first + 24 + 21 < 48 for first in (0, 1, 2)) and not 0 + 24 + 21 < 45     # grad_partial_sum's second trip
    for name in A.STRESS_STATES:                                       # make_state's own seeds and recipe
        n, k = A.STATES[name][:2]
        rng = np.random.default_rng(1000 + 10 * n + k)
        assert np.array_equal(A.make_state(name).Z, rng.normal(size=(n, k)))


def test_states_reach_every_kernel_form_and_reuse_the_ucb_states():
    padded = {name: -(-s[0] // 64) for name, s in A.STATES.items()}
    fast = {nb for name, nb in padded.items() if A.STATES[name][1] <= 40 and nb <= 8}
    assert fast == set(range(1, 9))                                    # every live k_acq_fast<SLAB, NB>
    assert padded["n513"] == 9 and A.STATES["k128"][1] == 128 and A.STATES["D"][1] == 41
    assert [A.STATES[n][1] for n in ("n64", "n65", "n129", "n193", "n257", "n321", "n385")] == [1, 3, 8, 9, 40, 1, 3]
    ucb = {"A": (9, 1, 1.0, "matern52"), "B": (70, 6, 1.0, "matern52"), "B-rbf": (70, 6, 1.0, "rbf"),
           "C": (449, 10, 1.0, "matern52"), "D": (50, 41, 1.0, "matern52"), "E": (30, 3, 1e-7, "matern52")}
    for name, shape in ucb.items():                                    # STATES of test_gpu_ucb.py, and its recipe
        assert A.STATES[name][:4] == shape
        n, k, yscale, _ = shape
        rng = np.random.default_rng(1000 + 10 * n + k)
        st = A.make_state(name)
        assert np.array_equal(st.Z, rng.normal(size=(n, k)))
        assert np.array_equal(st.y, (rng.normal(size=n) * 30.0 + 200.0) * yscale)
