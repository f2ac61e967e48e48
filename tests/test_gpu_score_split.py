"""pcabo_gp_condition_end_eval on two streams (PCABO_OPT_HIDDEN_TAIL, the default): the raw samples' copy and their kernel vectors
(k_score_ks_only) run on the context's second stream beside the factorisation, the mu_s sums (k_score_mu), k_score_gemm and
k_acq_combine follow behind alpha on the main stream.  The values must be, byte for byte, those of the parent's order -
pcabo_gp_condition_end, then pcabo_acq_eval, whose k_score_ks forms the kernel vectors and the mu_s sums in one kernel on one
stream - because every element keeps its operations and their order.

q: PCABO_INLAUNCH_MAXQ + 1 (read from csrc/pcabo_internal.h) is the smallest q for which pcabo_gp_condition_end_eval enqueues
behind the conditioning at all; up to 63 it takes the slab kernels (one stream, as before), from 64 on the GEMM path that is
split.  64 is one 64-sample tile exactly, 512 the raw samples of a BO iteration."""
import os
import re

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "para-ortho-pca-bo_amd", "csrc", "pcabo_internal.h")) as fh:
    INLAUNCH_MAXQ = int(re.search(r"#define\s+PCABO_INLAUNCH_MAXQ\s+(\d+)", fh.read()).group(1))
QS = (INLAUNCH_MAXQ + 1, 64, 512)
RUNGS = (0.0, 1e-8, 1e-7, 1e-6)


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=256, max_d=40, max_q=512)
    yield c
    c.close()


def _inputs(n, k):
    rng = np.random.default_rng([n, k, 4])
    Z = rng.uniform(-2.0, 2.0, (n, k))
    y = rng.normal(size=n) * 3.0 + 10.0
    Xq = rng.uniform(Z.min(0) - 0.3, Z.max(0) + 0.3, (max(QS), k))
    return Z, y, Xq


def retry_case():
    """n = 130, noise 0, two points duplicated (eight copies each, on both sides of the 64-row tile boundary): K is singular up
    to rounding, fourteen pivots are rounding noise around 0, and rung 0 of the jitter ladder fails at the first of them that is
    not positive.  tests/test_gp_reference_cpu.py-style check on the CPU (numpy restatement): see test_retry_case_needs_jitter."""
    rng = np.random.default_rng(1307)
    Z = rng.uniform(-1.0, 1.0, (130, 3))
    for i in (5, 20, 37, 66, 81, 99, 127):
        Z[i] = Z[2]
    for i in (9, 30, 63, 64, 70, 111, 128):
        Z[i] = Z[3]
    y = rng.normal(size=130) * 200.0 + 900.0
    Xq = rng.uniform(-1.2, 1.2, (512, 3))
    return Z, y, Xq


def test_retry_case_needs_jitter():
    """No GPU: the numpy restatement of the conditioning (tests/gp_reference.py) cannot factor the retry case's K at rung 0 and
    can at 1e-8."""
    from types import SimpleNamespace
    import gp_reference as G
    Z, y, _ = retry_case()
    case = SimpleNamespace(Z=Z, y=y, lengthscale=G.LENGTHSCALE, noise=0.0, kernel="matern", norm_bounds=None)
    with pytest.raises(np.linalg.LinAlgError):
        G.restate(case)
    assert np.isfinite(G.restate(case, jitter=1e-8).alpha).all()


def _rung(ctx):
    st = ctx.gp_state()
    seen = float(np.median(np.diag(st["L"] @ st["L"].T) - np.diag(ctx.gram())))
    return min(RUNGS, key=lambda r: abs(r - seen)), seen


def _split_and_parent(native, ctx, Z, y, Xq, scalar, acq, noise):
    ctx.set_option(native.OPT_HIDDEN_TAIL, 1)
    ctx.gp_condition(y, Z=Z, noise=noise, wait=False)
    split = ctx.gp_wait_eval(Xq, scalar, acq=acq)
    rung_split = _rung(ctx)[0]
    fresh = ctx.acq_eval(Xq, scalar, acq=acq, grad=False)        # the same model, k_score_ks in one piece
    ctx.set_option(native.OPT_HIDDEN_TAIL, 0)
    try:
        ctx.gp_condition(y, Z=Z, noise=noise, wait=False)
        ctx.gp_wait()
        parent = ctx.acq_eval(Xq, scalar, acq=acq, grad=False)
        rung_parent = _rung(ctx)[0]
    finally:
        ctx.set_option(native.OPT_HIDDEN_TAIL, 1)
    return split, fresh, parent, rung_split, rung_parent


@gpu
@pytest.mark.parametrize("acq", ["log_ei", "ucb"])
@pytest.mark.parametrize("k", [1, 36])
@pytest.mark.parametrize("n", [65, 200])
def test_two_stream_scoring_has_the_parents_bytes(native, ctx, n, k, acq):
    Z, y, Xq = _inputs(n, k)
    code, scalar = (native.ACQ_LOG_EI, float(y.min())) if acq == "log_ei" else (native.ACQ_UCB, 1.5)
    for q in QS:
        split, fresh, parent, _, _ = _split_and_parent(native, ctx, Z, y, Xq[:q], scalar, code, 1e-4)
        assert np.isfinite(parent).all()
        assert split.tobytes() == parent.tobytes(), (n, k, acq, q, np.abs(split - parent).max())
        assert split.tobytes() == fresh.tobytes(), (n, k, acq, q)


@gpu
@pytest.mark.parametrize("acq", ["log_ei", "ucb"])
def test_scores_behind_a_jitter_retry(native, ctx, acq):
    """The factorisation fails at rung 0: R and alpha are computed again with jitter and only the launches behind them run again
    (the kernel vectors on the second stream do not depend on the jitter).  Same rung as the one-stream path, same bytes, and
    equal to a fresh evaluation of the conditioned model."""
    Z, y, Xq = retry_case()
    code, scalar = (native.ACQ_LOG_EI, float(y.min())) if acq == "log_ei" else (native.ACQ_UCB, 1.5)
    split, fresh, parent, rung_split, rung_parent = _split_and_parent(native, ctx, Z, y, Xq, scalar, code, 0.0)
    assert rung_parent > 0.0, "the one-stream path factored the retry case at rung 0: the retry was not exercised"
    assert rung_split == rung_parent
    assert split.tobytes() == parent.tobytes()
    assert split.tobytes() == fresh.tobytes()
