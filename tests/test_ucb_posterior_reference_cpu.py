"""The extended-precision reference of UCB and of the posterior query and its error units, proved without a GPU.

`test_gpu_ucb_edges.py` and `test_gpu_posterior_edges.py` hold the HIP kernels to 16 of the units of `acq_reference`
(`scalars_ucb`, `posterior`).  As for log-EI and PI (`test_acq_reference_cpu.py`) that is only worth something if an
independent fp64 implementation written as the kernels are - `acq_reference.restate` with acq = UCB and
`acq_reference.restate_posterior`: numpy, direct distances, the 1e-30 guard, V = R KS^T, V^T V - stays well inside them
(limit 4) on conditioned states of `gp_reference.restate`, and if wrong variants of it leave them (more than 16) on the
states named beside each variant.  The same file asserts what the device tests rely on: the hand-placed queries, the
near-coincident pairs, no variance - latent or with the observation noise - within rounding of the 1e-10 floor.
"""
import numpy as np
import pytest

import acq_reference as A

LIMIT = 4.0
DEVICE_LIMIT = 16.0
PROVED_UCB = A.SMALL_STATES + ["C"] + A.STRESS_STATES      # as test_acq_reference_cpu.py: n <= 130, n = 449, the stress states
PROVED_POSTERIOR = A.POSTERIOR_STATES      # every state of the device test
_UCB, _POST = {}, {}


def _ucb_refs(name):
    if name not in _UCB:
        _, _, lin = A.prepared(name)
        _UCB[name] = {label: (mx, kap, A.scalars(lin, kap, mx, A.UCB)) for label, _, mx, kap in A.cases_ucb(lin)}
    return _UCB[name]


def _post_ref(name, noise):
    if (name, noise) not in _POST:
        st, _, lin = A.prepared(name)
        _POST[name, noise] = A.posterior(st, lin, noise)
    return _POST[name, noise]


@pytest.mark.parametrize("name", PROVED_UCB)
def test_ucb_restatement_within_units(name, capsys):
    """Value and every gradient component of the fp64 restatement at all 130 queries, 4 kappas x 2 directions: <= 4."""
    st, gs, _ = A.prepared(name)
    worst, bad = [0.0, 0.0], []
    for label, (mx, kap, ref) in _ucb_refs(name).items():
        rv, rg = A.judge(ref, *A.restate(st, gs, st.X, kap, mx, A.UCB))
        worst = [max(worst[0], rv), max(worst[1], rg)]
        if not (rv <= LIMIT and rg <= LIMIT):
            bad.append((label, rv, rg))
    with capsys.disabled():
        print("\n[UCB, fp64 restatement / reference units, state %s (n=%d k=%d %s)] worst value %.3g gradient %.3g"
              % (name, st.n, st.k, st.kernel, worst[0], worst[1]))
    assert not bad, bad


@pytest.mark.parametrize("name", PROVED_POSTERIOR)
def test_posterior_restatement_within_units(name, capsys):
    """Mean, floored variance and all 130 x 130 covariance entries of the fp64 restatement, both noise flags: <= 4; the
    floored variances are exactly 1e-10 (their unit is 0) and the covariance is symmetric bit for bit."""
    st, gs, _ = A.prepared(name)
    worst, bad = {}, []
    for noise in (False, True):
        out = A.restate_posterior(st, gs, st.X, noise)
        for key, r in A.judge_posterior(_post_ref(name, noise), out).items():
            worst[key] = max(worst.get(key, 0.0), r)
            if not r <= LIMIT:
                bad.append((noise, key, r))
    with capsys.disabled():
        print("\n[posterior, fp64 restatement / reference units, state %s (n=%d k=%d %s)] worst mean %.3g variance %.3g "
              "covariance %.3g" % (name, st.n, st.k, st.kernel, worst["mean"], worst["variance"], worst["covariance"]))
    assert not bad, bad


@pytest.mark.parametrize("variant", list(A.WRONG_UCB))
def test_units_notice_wrong_ucb_variant(variant, capsys):
    """Each wrong variant of the UCB restatement leaves the device's limit of 16 on every state named beside it."""
    kw, what, kappas, states = A.WRONG_UCB[variant]
    seen, bad = [], []
    for name in states:
        st, gs, _ = A.prepared(name)
        worst = 0.0
        for label, (mx, kap, ref) in _ucb_refs(name).items():
            if kap in kappas:
                rv, rg = A.judge(ref, *A.restate(st, gs, st.X, kap, mx, A.UCB, **kw))
                worst = max(worst, {"value": rv, "grad": rg, "any": max(rv, rg)}[what])
        seen.append("%s %.3g" % (name, worst))
        if not worst > DEVICE_LIMIT:
            bad.append((name, worst))
    with capsys.disabled():
        print("\n[UCB, %s: worst %s ratio per state] %s" % (variant, what, "; ".join(seen)))
    assert not bad, bad


@pytest.mark.parametrize("variant", list(A.WRONG_POSTERIOR))
def test_units_notice_wrong_posterior_variant(variant, capsys):
    """Each wrong variant of the posterior restatement leaves the device's limit of 16 on every state named beside it.
    The query-query distance as norms minus a dot product must do so at the covariance of the duplicate pair (3, 4)
    AND at that of a near-coincident pair, nowhere else: away from them the kernel's slope in sq is small and the unit
    of v_a . v_b wide.  It is seen where |xn|^2 / l^2 is large: one rounding of the norms at k = 128 is 28 units there,
    at k = 41 (state D) one is 7 and below the limit - the norm form IS nearly as good as the direct one at small k.
    Every other variant that needs no clamped variance is also held on the stress state n385k65; this one is not named
    there: at lengthscale 2.0 and with the unit of v_a . v_b summed over 385 rows it stays at 0.014 of the unit."""
    kw, flags, states = A.WRONG_POSTERIOR[variant]
    seen, bad = [], []
    for name in states:
        st, gs, _ = A.prepared(name)
        for noise in flags:
            ref = _post_ref(name, noise)
            out = A.restate_posterior(st, gs, st.X, noise, **kw)
            worst = max(A.judge_posterior(ref, out).values())
            seen.append("%s%s %.3g" % (name, "+noise" if noise else "", worst))
            if not worst > DEVICE_LIMIT:
                bad.append((name, noise, worst))
            if "qq_norms" in kw:
                with np.errstate(invalid="ignore", divide="ignore"):
                    e = np.abs(A.f64(A.hp(out["covariance"]) - ref.covariance)) / ref.u_covariance
                dup, near = float(e[3, 4]), max(float(e[a, b]) for a, b in A.NEAR_PAIRS)
                seen.append("(duplicate %.3g, near-coincident %.3g)" % (dup, near))
                if not (dup > DEVICE_LIMIT and near > DEVICE_LIMIT):
                    bad.append((name, noise, "pairs", dup, near))
    with capsys.disabled():
        print("\n[posterior, %s: worst ratio per state] %s" % (variant, "; ".join(seen)))
    assert not bad, bad


def test_the_diagonal_variants_are_seen_on_the_diagonal_only():
    """The covariance's diagonal from the tile product is wrong only under the noise flag (the epilogue's prior has no
    s2 delta_ab); without it, it is the same sum in another order and stays inside the variance's unit - so that
    variant is no error there, and the test of the device cannot and need not tell the two apart."""
    for name in ("A", "B", "user"):
        st, gs, _ = A.prepared(name)
        out = A.restate_posterior(st, gs, st.X, False, diag_from_tile=True)
        assert max(A.judge_posterior(_post_ref(name, False), out).values()) <= LIMIT, name


@pytest.mark.parametrize("name", list(A.STATES))
def test_case_inputs_satisfy_the_conditions_of_the_device_tests(name):
    """UCB on every state; the posterior's conditions on its own states: the queries of test_acq_reference_cpu.py, the
    followers of NEAR_PAIRS 1e-9 off their leaders (in every prefix from 15 on, and across two covariance tiles at 130),
    the duplicate pair, no latent or noisy variance within 32 dvar of the floor, every clamped variance decisively so."""
    st, _, lin = A.prepared(name)
    assert [len(A.cases_ucb(lin)), len({c[0] for c in A.cases_ucb(lin)})] == [8, 8]
    assert {c[3] for c in A.cases_ucb(lin)} == {0.0, 0.5, 2.0 ** 0.5, 1e3}
    assert A.check_ucb_conditions(name, st, lin) == []
    if name in A.POSTERIOR_STATES:
        assert A.check_posterior_conditions(name, st, lin) == []
    assert not set(st.redrawn) & ({b for _, b in A.NEAR_PAIRS} | set(A.FIXED_QUERIES))
    assert A.NEAR_PAIRS == ((6, 7), (4, 129)) and A.POST_PREFIXES == (1, 15, 16, 17, 63, 64, 65, 130)


def test_posterior_states_reach_the_forms_the_device_test_names():
    assert set(A.SMALL_STATES) <= set(A.POSTERIOR_STATES)
    assert {"n257", "n513", "D", "k128", "user", "E", "mixed"} <= set(A.POSTERIOR_STATES)
    assert set(A.STRESS_STATES) <= set(A.POSTERIOR_STATES) and not set(A.STRESS_STATES) & set(A.SMALL_STATES)
    for variants in (A.WRONG_UCB, A.WRONG_POSTERIOR):                  # the wrong variants are seen in the stress region too
        assert any("n385k65" in v[-1] for v in variants.values())
    for name, floor in (("E", "all"), ("mixed", "some")):
        st, _, lin = A.prepared(name)
        for noise in (False, True):
            cl = A.posterior(st, lin, noise).clamped
            assert cl.all() if floor == "all" else (cl.any() and not cl.all()), (name, noise)
