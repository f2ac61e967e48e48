"""No GPU: what every input of tests/batch_rare_cases.py is there for, shown on the numpy restatement of the conditioning
(gp_reference.restate) and the oracle's weighted PCA, so that tests/test_gpu_batch_rare_paths.py never depends on a case that does
not do what it is used for.

A margin is the smallest pivot of the factorisation over n eps ||K||_2; 1e3 of it, as test_gp_reference_cpu.py asks of the ladder
cases, puts a factorisation out of rounding's reach: below it "rung 0 goes either way", above it it does not.
"""
import numpy as np
import pytest

import batch_rare_cases as BC
import extend_reference as ER
import gp_reference as G
import pcabo_oracle as O
from wpca_reference import hp

BIG_B = 86                                                         # the oversubscribed batch takes plain(0 .. 85)


def _fails(case, jitter=0.0):
    with pytest.raises(np.linalg.LinAlgError):
        G.restate(case, jitter=jitter)


def _climbs(case):
    """Rung 0 fails, 1e-8 factors with the margin and it is that rung which makes it so."""
    _fails(case)
    margin = BC.pivot_margin(case, 1e-8)
    assert margin >= BC.MARGIN, (case.id, margin)
    res = G.restate(case, jitter=1e-8)
    assert np.linalg.eigvalsh(res.K)[0] < BC.MARGIN * case.n * BC.EPS * np.linalg.norm(res.K, 2), case.id
    assert np.isfinite(res.alpha).all()
    return margin


def test_retry_leaves_rung_zero_and_factors_at_the_next(capsys):
    """retry: K singular up to rounding (fourteen copies), 1e-8 decisively enough."""
    case = BC.retry()
    assert (case.n, case.k, case.noise) == (BC.N, BC.K, 0.0)
    for rows, src in ((BC.DUP_A, 2), (BC.DUP_B, 3)):
        assert all(np.array_equal(case.Z[i], case.Z[src]) for i in rows)
    assert min(BC.DUP_A + BC.DUP_B) < 64 <= max(BC.DUP_A + BC.DUP_B)     # copies on both sides of the tile boundary
    margin = _climbs(case)
    with capsys.disabled():
        print("\nretry: rung 0 fails, smallest pivot at 1e-8 = %.3g n eps ||K||" % margin)


def test_retry_tail_leaves_rung_zero_too(capsys):
    """tail: the 64 + 66 rows used at ld > NP - six copies in the first tile are enough."""
    case = BC.retry_tail()
    assert np.array_equal(case.Z[:64], BC.retry().Z[:64]) and not np.array_equal(case.Z[64:], BC.retry().Z[64:])
    assert len(np.unique(case.Z[64:], axis=0)) == BC.N - 64
    margin = _climbs(case)
    with capsys.disabled():
        print("\nretry-tail: rung 0 fails, smallest pivot at 1e-8 = %.3g n eps ||K||" % margin)


def test_plain_runs_factor_at_rung_zero_with_margin(capsys):
    """plain(0 .. 85) and the tail's donor: smallest pivot >= 1e3 n eps ||K|| at rung 0, every run with data of its own."""
    seeds = list(range(BIG_B)) + [77]
    margins = {s: BC.pivot_margin(BC.plain(s)) for s in seeds}
    assert min(margins.values()) >= BC.MARGIN, min(margins.items(), key=lambda kv: kv[1])
    assert len({BC.plain(s).Z.tobytes() for s in seeds}) == len(set(seeds))
    with capsys.disabled():
        print("\nplain: smallest pivot at rung 0 >= %.3g n eps ||K|| over %d runs" % (min(margins.values()), len(seeds)))


def test_dead_has_no_rung():
    """dead: finite inputs, but the zero-range column makes every entry of K NaN (0 / 0 in Normalize) - the first pivot of the
    reference's Cholesky is not positive on any rung, and no jitter on the diagonal changes a NaN."""
    case = BC.dead(1)
    assert np.ptp(case.Z[:, BC.DEAD_COLUMN]) == 0.0 and np.isfinite(case.Z).all() and np.isfinite(case.y).all()
    K = G.gram_reference(case).K
    assert np.isnan(G.f64(K)).all()
    for jitter in G.RUNGS:
        with pytest.raises(G.NotPositiveDefinite, match="pivot 1 "):
            G.hp_cholesky(K + hp(jitter) * hp(np.eye(case.n)))
    assert BC.pivot_margin(BC.plain(1)) >= BC.MARGIN               # the same points with the column left alone do factor


def test_wpca_inputs_give_different_k_and_a_middle_run_that_climbs(capsys):
    """The fused route: the oracle's weighted PCA gives k = 5, 3, 4; the middle run's projected points have the exact duplicates
    of its X, fail rung 0 and factor at 1e-8; the outer runs factor at rung 0 with the margin."""
    X, y, ranks, noise = BC.wpca_inputs()
    lines = []
    for b in range(3):
        w = O.weighted_pca(X[b], y[b], False, BC.VAR_THRESHOLD, 0, noise=noise[b], ranks=ranks[b])
        assert w.k == BC.WPCA_K[b], (b, w.k, w.evr)
        case = BC.as_case(w.Z, y[b], "wpca%d" % b)
        if b == 1:
            assert all(np.array_equal(w.Z[i], w.Z[2]) for i in BC.DUP_A) and all(np.array_equal(w.Z[i], w.Z[3]) for i in BC.DUP_B)
            margin = _climbs(case)
        else:
            margin = BC.pivot_margin(case)
            assert margin >= BC.MARGIN, (b, margin)
        lines.append("  run %d: k = %d, %s, margin %.3g" % (b, w.k, "rung 1e-8" if b == 1 else "rung 0", margin))
    with capsys.disabled():
        print("\nwPCA inputs\n" + "\n".join(lines))


def test_the_likelihood_domain_admits_a_noise_at_which_retry_climbs():
    """pcabo_batch_gp_mll asks s2 > 0 and finite (mll_theta_ok): 1e-300 is inside, and 1 + 1e-300 == 1, so K is the K of noise 0
    byte for byte and rung 0 fails as it does there.  softplus(0) = ln 2 is the conditioning's lengthscale."""
    case = BC.retry()
    k0 = G.restate(case, jitter=1e-8).K
    case.noise = 1e-300
    assert case.noise > 0.0 and np.isfinite(case.noise) and 1.0 + case.noise == 1.0
    _fails(case)
    assert G.restate(case, jitter=1e-8).K.tobytes() == k0.tobytes()
    assert np.log1p(np.exp(0.0)) == G.LENGTHSCALE


def test_the_extend_reference_notices_a_pivot_formed_without_the_rung(capsys):
    """retry at rung 1e-8, extended by three uniform points: the bordering step in fp64 with the diagonal 1 + s2 + rung stays
    inside one unit of extend_reference.step(rung=1e-8) on the same R; with the rung left out of d2 the new rows of L and R leave
    the limit of 16 - 1e-8 is far above the unit of d2 there, so the device test can tell the two apart."""
    case = BC.retry()
    res = G.restate(case, jitter=1e-8)
    Xp, _ = BC.new_points(case, 3)
    R, Z, lines = res.R, case.Z, []
    for i in range(3):
        b = ER.step(R, Xp[i], Z, res.norm_bounds, case.lengthscale, case.noise, case.kernel, rung=1e-8)
        ks = ER.kernel_vector_f64(Xp[i], Z, res.norm_bounds, case.lengthscale, case.kernel)
        good, bad = ER.border_f64(R, ks, 1.0 + case.noise + 1e-8), ER.border_f64(R, ks, 1.0 + case.noise)
        assert good is not None and bad is not None
        assert float(b.d2) > 1e3 * 1e-8                             # no pivot near the rung's own size: d2 is not a rounding difference
        ratios = {(name, row): ER.ratio(hp(getattr(v, row)) - getattr(b, row), getattr(b.units, row))
                  for name, v in (("good", good), ("bad", bad)) for row in ("L_row", "R_row")}
        assert max(ratios["good", "L_row"], ratios["good", "R_row"]) <= 1.0, ratios
        assert min(ratios["bad", "L_row"], ratios["bad", "R_row"]) > ER.LIMIT, ratios
        lines.append("  point %d: d2 %.3e (unit %.1e)  with the rung %.3g / %.3g units, without %.0f / %.0f"
                     % (i, float(b.d2), b.units.d2, ratios["good", "L_row"], ratios["good", "R_row"], ratios["bad", "L_row"],
                        ratios["bad", "R_row"]))
        n = R.shape[0]
        grown = np.zeros((n + 1, n + 1))
        grown[:n, :n], grown[n] = R, good.R_row
        R, Z = grown, np.vstack([Z, Xp[i:i + 1]])
    with capsys.disabled():
        print("\nextend at rung 1e-8, rows of L / R in extend_reference units\n" + "\n".join(lines))
