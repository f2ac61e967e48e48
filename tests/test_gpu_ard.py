"""The GP fit with one lengthscale per input on the MI355X (pcabo_gp_mll_ard / pcabo_gp_fit_ard: k_mll_grad<true>, k_mll_finish<true> and
the lengthscales folded into the Normalize ranges by k_zstats; PCA_BO / Vanilla_BO fit_gp=True, ard=True) against the restatement of
tests/ard_reference.py (torch float64 autograd + scipy's L-BFGS-B).

Shapes (n, k): one padded tile (9, 1), (40, 3); exactly one tile (64, 4); an off-diagonal tile with a single live row (65, 5); three
block rows (130, 9); KP padding of 1 to 3; k across 64 (70, 33), (70, 65); n < k (20, 100); k = PCABO_MAXD (129, 128).

Caps, those tests/test_gpu_gp_fit.py states for the scalar fit (fixed beforehand, not fitted to the device): loss 1e-9 relative to
max(|loss|, 1e-2), every gradient component 1e-7 relative to max(|g|, 1e-3 x the sum of absolute values of its terms).
Measured on an MI355X: see EXPERIMENTS.md "ARD lengthscales" (the first test prints the worst ratios).

The gradient cap is relative to 1e-3 of a term scale; every S_c in first-order error units of a long-double reference, at the
shapes where KP, the chunks of eight and the tiles change: tests/test_gpu_mll_edges.py (reference and units: tests/mll_reference.py).
"""
import math

import numpy as np
import pytest

import pcabo_oracle as O
from ard_reference import EVAL_ONLY_STATE, FIT_STATES, ArdFit, ard_state, fitted_gp, theta0
from pcabo.bbob import BBOBProblem
from test_gp_fit_cpu import RestatedFit
from ucb_reference import UCBReference, kappa_of

pytestmark = pytest.mark.gpu

LOSS_CAP, GRAD_CAP = 1e-9, 1e-7
SEEDS = {(40, 3): 1, (65, 5): 2, (70, 33): 4, (130, 9): 3}         # the issue's states where a shape is one of them
SHAPES = [(9, 1), (40, 3), (64, 4), (65, 5), (130, 9), (70, 33), (70, 65), (20, 100), (129, 128)]
assert EVAL_ONLY_STATE == (3, 130, 9) and all(SEEDS[(n, k)] == s for s, n, k in FIT_STATES)


def _state(n, k):
    return ard_state(SEEDS.get((n, k), 100 + n + k), n, k)


def _thetas(n, k):
    """The start; seeded rho in [-1.5, 2] with c != 0; the noise at its bound; one rho_c = 15; one rho_c = 25 (softplus's linear
    branch)."""
    rng = np.random.default_rng(1000 * n + k)
    rho = rng.uniform(-1.5, 2.0, size=k)
    c = int(rng.integers(k))
    big, lin = rho.copy(), rho.copy()
    big[c], lin[c] = 15.0, 25.0
    return [theta0(k), np.r_[0.05, 0.3, rho], np.r_[1e-4, -0.2, rho], np.r_[0.05, 0.3, big], np.r_[0.02, -0.1, lin]]


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=130, max_d=128, max_q=512)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fit_states():
    return {(n, k): ard_state(seed, n, k) for seed, n, k in FIT_STATES}


@pytest.fixture(scope="module")
def fits(ctx, fit_states):
    """One device ARD fit per fit state (shared; the tests that need the context conditioned there fit again)."""
    return {key: ctx.gp_fit_ard(y, Z=Z) for key, (Z, y) in fit_states.items()}


def test_gp_mll_ard_matches_the_restated_loss_and_gradient(ctx, capsys):
    worst_l, worst_g, rows = 0.0, 0.0, []
    for n, k in SHAPES:
        Z, y = _state(n, k)
        ref = ArdFit(Z, y)
        wl = wg = 0.0
        for theta in _thetas(n, k):
            r = ctx.gp_mll_ard(y, theta, Z=Z)
            lv, lg = ref.value_and_grad(theta)
            el = abs(r["loss"] - lv) / max(abs(lv), 1e-2)
            eg = np.abs(r["grad"] - lg) / np.maximum(np.abs(lg), 1e-3 * ref.term_scales(theta))
            wl, wg = max(wl, el), max(wg, float(eg.max()))
            print(f"  (n, k) = ({n}, {k}) theta[:2] = {theta[:2]}: loss {el:.2e}, gradient {eg.max():.2e} (component {int(eg.argmax())})")
            assert r["grad"].shape == (2 + k,) and r["lengthscales"].shape == (k,)
            assert el <= LOSS_CAP, (n, k, theta, r["loss"], lv)
            assert (eg <= GRAD_CAP).all(), (n, k, theta, int(eg.argmax()), r["grad"][eg.argmax()], lg[eg.argmax()])
        rows.append((n, k, wl, wg))
        worst_l, worst_g = max(worst_l, wl), max(worst_g, wg)
    with capsys.disabled():
        print("\n  gp_mll_ard vs restatement, worst relative error per shape (loss, gradient): "
              + "  ".join(f"({n},{k}) {a:.1e} {b:.1e}" for n, k, a, b in rows))
        print(f"  overall: loss {worst_l:.2e} (cap {LOSS_CAP:.0e}), gradient {worst_g:.2e} (cap {GRAD_CAP:.0e})")


def test_equal_rho_is_the_scalar_fit(ctx):
    for n, k in SHAPES:
        Z, y = _state(n, k)
        for s2, c, rho in ((math.exp(-5.0), 0.0, 0.0), (1e-4, 0.3, -0.5), (0.05, -0.2, 0.8)):
            sc = ctx.gp_mll(y, (s2, c, rho), Z=Z)
            ar = ctx.gp_mll_ard(y, np.r_[s2, c, np.full(k, rho)], Z=Z)
            scale = RestatedFit(Z, y).term_scales((s2, c, rho))
            assert abs(ar["loss"] - sc["loss"]) <= LOSS_CAP * max(abs(sc["loss"]), 1e-2), (n, k, rho)
            g3 = np.r_[ar["grad"][:2], ar["grad"][2:].sum()]
            err = np.abs(g3 - sc["grad"]) / np.maximum(np.abs(sc["grad"]), 1e-3 * scale)
            assert (err <= GRAD_CAP).all(), (n, k, rho, g3, sc["grad"])


def test_two_evaluations_and_two_fits_are_bit_identical(native, fit_states, fits):
    for (n, k), (Z, y) in fit_states.items():
        out = [fits[(n, k)]]
        c = native.Context(max_n=n, max_d=k, max_q=64)         # another context, of another capacity
        try:
            out.append(c.gp_fit_ard(y, Z=Z))
            again = c.gp_mll_ard(y, out[-1]["theta"], Z=Z)
            once_more = c.gp_mll_ard(y, out[-1]["theta"], Z=Z)
        finally:
            c.close()
        a, b = out
        assert a["theta"].tobytes() == b["theta"].tobytes(), (n, k)
        assert a["loss"] == b["loss"]
        assert [a[key] for key in ("iterations", "evaluations", "warnflag", "task")] == \
            [b[key] for key in ("iterations", "evaluations", "warnflag", "task")]
        assert again["loss"] == b["loss"], "the returned loss is gp_mll_ard's at the returned theta, bit for bit"
        assert again["grad"].tobytes() == once_more["grad"].tobytes()


def test_fits_beat_the_scalar_fit(ctx, fit_states, fits, capsys):
    rows = []
    for (n, k), (Z, y) in fit_states.items():
        r = fits[(n, k)]
        assert "lengthscale" not in r and r["lengthscales"].shape == (k,)
        lv, _ = ArdFit(Z, y).value_and_grad(r["theta"])
        assert abs(r["loss"] - lv) <= LOSS_CAP * max(abs(lv), 1e-2), (n, k, r["loss"], lv)
        sc = ctx.gp_fit(y, Z=Z)
        rows.append((n, k, sc["loss"], r, r["lengthscales"]))
        assert r["loss"] <= sc["loss"] - 0.25, (n, k, r["loss"], sc["loss"])
    with capsys.disabled():
        print()
        for n, k, ls, r, lsc in rows:
            print(f"  (n, k) = ({n}, {k}): scalar fit loss {ls:.3f}, ARD fit loss {r['loss']:.5f} ({r['iterations']} it / "
                  f"{r['evaluations']} ev, warnflag {r['warnflag']}, task {r['task']}), lengthscales "
                  f"{np.array2string(lsc[:2], precision=3)} then {lsc[2:].min():.1f} .. {lsc[2:].max():.1f}")


@pytest.mark.parametrize("n,k", [(n, k) for _, n, k in FIT_STATES])
def test_fits_end_with_warnflag_0(fits, n, k):
    """Measured on an MI355X: (40, 3) 62 iterations / 90 evaluations, loss 0.36333; (65, 5) 34 / 63, -0.01364 (the reference fit:
    45 / 72, -0.01575); (70, 33) 131 / 175, -0.09942 (reference fit: 78 / 109, -0.0911; the scalar fit: 1.350); all warnflag 0.
    The fit bounds every rho_c below by ln 2^-40.  Without that bound the (70, 33) fit ended with warnflag 2, task
    PCABO_FIT_TASK_DOMAIN, after 92 / 123 at -0.09252: a line-search trial with rho_c = -4759, softplus(rho_c) = 0.  The flat
    directions make the path sensitive to the last bits of the gradient: of eight CPU reference fits with the gradient perturbed
    by 1e-13, one runs into such a trial (rho_c = -614) and seven end at -0.0994, where the device fit now ends."""
    r = fits[(n, k)]
    assert r["warnflag"] == 0, (r["warnflag"], r["task"], r["iterations"], r["evaluations"], r["loss"])


def _close(v, ov, g=None, og=None):
    assert (np.abs(v - ov) / np.maximum(1.0, np.abs(ov))).max() < 1e-8
    if g is not None:
        assert np.abs(g - og).max() < 1e-7 * max(1.0, np.abs(og).max())


def test_acquisition_after_the_fit_uses_the_fitted_model(native, ctx, fit_states):
    grp = native.Context(max_n=130, max_d=33, max_q=64)
    grp.set_option(native.OPT_GROUP_ACQ, 1)
    try:
        for (n, k), (Z, y) in fit_states.items():
            r = ctx.gp_fit_ard(y, Z=Z)
            assert grp.gp_fit_ard(y, Z=Z)["theta"].tobytes() == r["theta"].tobytes()
            gp = fitted_gp(Z, y, r)
            box = O.acq_bounds(Z)
            assert np.array_equal(ctx.acq_bounds(), box) or np.abs(ctx.acq_bounds() - box).max() < 1e-12   # never folded
            X = np.random.default_rng(7).uniform(box[0], box[1], size=(512, k))
            best_f, kappa = float(np.min(y)), kappa_of(2.0)
            for scalar, code, ref in ((best_f, native.ACQ_LOG_EI, O.Acquisition(gp, best_f, False)),
                                      (kappa, native.ACQ_UCB, UCBReference(gp, 2.0, False))):
                ov, og = ref.value_and_grad(X)
                v, g = ctx.acq_eval(X[:64], scalar, False, code)
                _close(v, ov[:64], g, og[:64])
                _close(ctx.acq_eval(X, scalar, False, code, grad=False), ov)                  # q = 512: GEMM scoring
                for q in (5, 32):
                    vg, gg = grp.acq_eval(X[:q], scalar, False, code)                         # k_acq_group
                    _close(vg, ov[:q], gg, og[:q])
                cand, vals, info, failed = ctx.optimize_acqf(X[:10], box, scalar, False, code)
                _close(vals, ctx.acq_eval(cand, scalar, False, code, grad=False))
                _close(vals, ref.value_and_grad(cand)[0])
    finally:
        grp.close()


def test_the_next_conditioning_returns_to_the_unfolded_model(native, ctx, fit_states):
    Z, y = fit_states[(65, 5)]
    r = ctx.gp_fit_ard(y, Z=Z)
    folded = ctx.gp_state()["norm_bounds"]
    nb = O.normalize_bounds(Z)
    assert np.allclose(folded[0], nb[0], rtol=1e-15, atol=0)
    assert np.allclose(folded[1] - folded[0], (nb[1] - nb[0]) * r["lengthscales"], rtol=1e-14, atol=0)
    ctx.gp_condition(y, Z=Z)
    fresh = native.Context(max_n=130, max_d=128, max_q=512)
    try:
        fresh.gp_condition(y, Z=Z)
        a, b = ctx.gp_state(), fresh.gp_state()
        for key in ("L", "R", "alpha", "norm_bounds"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert (a["y_mean"], a["y_std"]) == (b["y_mean"], b["y_std"])
        assert ctx.gram().tobytes() == fresh.gram().tobytes()
    finally:
        fresh.close()


def test_argument_errors(native, ctx, fit_states):
    Z, y = fit_states[(40, 3)]
    bad_thetas = (np.r_[0.0, 0.0, 0.0, 0.0, 0.0], np.r_[-1.0, 0.0, 0.0, 0.0, 0.0], np.r_[float("nan"), 0.0, 0.0, 0.0, 0.0],
                  np.r_[0.01, 0.0, 0.0, float("nan"), 0.0], np.r_[0.01, 0.0, 0.0, -800.0, 0.0])     # softplus(-800) = 0
    bt = native.Batch(2, max_n=40, max_d=3, max_q=64)
    try:
        calls = [lambda: ctx.gp_mll_ard(y, theta0(3), Z=Z, kernel=native.KERNEL_RBF),
                 lambda: ctx.gp_fit_ard(y, Z=Z, kernel=native.KERNEL_RBF),
                 lambda: bt.ctx[0].gp_mll_ard(y, theta0(3), Z=Z),                                  # a member context of a batch
                 lambda: bt.ctx[1].gp_fit_ard(y, Z=Z)]
        for bad in bad_thetas:
            calls.append(lambda t=bad: ctx.gp_mll_ard(y, t, Z=Z))
        for bad in bad_thetas[2:]:                             # (a start with s2 below its bound is clipped into the box, as scipy
            calls.append(lambda t=bad: ctx.gp_fit_ard(y, t, Z=Z))   # and pcabo_gp_fit do: see the end of this test)
        for call in calls:
            with pytest.raises(native.PcaboError) as e:
                call()
            assert e.value.code == -1
    finally:
        bt.close()
    assert ctx.gp_mll_ard(y, theta0(3), Z=Z)["loss"] == ctx.gp_mll_ard(y, theta0(3), Z=Z)["loss"]    # as usable as before
    clipped, at_bound = ctx.gp_fit_ard(y, bad_thetas[0], Z=Z), ctx.gp_fit_ard(y, np.r_[1e-4, 0.0, 0.0, 0.0, 0.0], Z=Z)
    assert clipped["theta"].tobytes() == at_bound["theta"].tobytes() and clipped["evaluations"] == at_bound["evaluations"]
    # the same for the fit's lower bound on rho_c, ln 2^-40: softplus(-100) > 0 is inside the domain and below the bound
    clipped, at_bound = (ctx.gp_fit_ard(y, np.r_[0.01, 0.0, 0.0, r, 0.0], Z=Z) for r in (-100.0, -40.0 * math.log(2.0)))
    assert clipped["theta"].tobytes() == at_bound["theta"].tobytes() and clipped["evaluations"] == at_bound["evaluations"]
    assert clipped["theta"][2:].min() >= -40.0 * math.log(2.0)


def test_pca_bo_run_with_ard():
    from Algorithms import PCA_BO
    opt = PCA_BO(budget=45, n_DoE=30, random_seed=15101, fit_gp=True, ard=True)
    opt(problem=BBOBProblem(15, 0, 10), dim=10, bounds=np.array([-5.0, 5.0]))
    assert math.isfinite(opt.current_best)
    hp = opt.gp_hyperparameters
    k = hp["theta"].shape[0] - 2
    assert hp["lengthscales"].shape == (k,) and k >= 2
    assert not np.all(hp["lengthscales"] == hp["lengthscales"][0]), hp


def test_vanilla_bo_run_with_ard():
    from Algorithms import Vanilla_BO
    opt = Vanilla_BO(budget=25, n_DoE=15, random_seed=15051, fit_gp=True, ard=True)
    opt(problem=BBOBProblem(15, 0, 5), dim=5, bounds=np.array([-5.0, 5.0]))
    assert math.isfinite(opt.current_best)
    hp = opt.gp_hyperparameters
    assert hp["lengthscales"].shape == (5,)
    assert not np.all(hp["lengthscales"] == hp["lengthscales"][0]), hp
