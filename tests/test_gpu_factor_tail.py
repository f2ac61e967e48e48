"""The root inverse folded into the Cholesky panel launches of a single context (PCABO_OPT_HIDDEN_TAIL, the default; DESIGN.md
section 4): wave 2 of panel group 0 inverts the diagonal block beside the pivot chain, launch J carries the groups of row block
J - 1 of R, one drain launch adds the last row block.  Option 0 selects the separate launches k_trinv_diag_w + k_trinv_cols behind
the last panel.  Every element of L, R and alpha keeps its operations and their order, so the two must agree byte for byte - the
whole n x n arrays as pcabo_get_gp_state returns them, upper triangles included - and so must acquisition values on top of them.

Shapes (NP = n rounded up to the 64-wide panel): n = 5 one panel, the diagonal inverse alone; 64 / 65 and 128 / 129 an exact tile
and a last block with one real row; 200 four panels - a row block computed beside a later panel while two more follow; 449 the
benchmark's last shape, once."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(n, k) for n in (5, 64, 65, 128, 129, 200) for k in (1, 4, 36)] + [(449, 36)]
RUNGS = (0.0, 1e-8, 1e-7, 1e-6)


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=449, max_d=40, max_q=16)
    yield c
    c.close()


def _inputs(n, k, seed=0):
    rng = np.random.default_rng([n, k, seed, 5])
    Z = rng.uniform(-2.0, 2.0, (n, k))
    y = rng.normal(size=n) * 3.0 + 10.0
    Xq = rng.uniform(Z.min(0) - 0.3, Z.max(0) + 0.3, (8, k))
    return Z, y, Xq


def _state_bytes(native, c):
    n = c.n
    L, R, alpha, ys = np.empty((n, n)), np.empty((n, n)), np.empty(n), np.empty(2)
    c._chk(native.LIB.pcabo_get_gp_state(c._h, *[a.ctypes.data_as(C.c_void_p) for a in (L, R, alpha, ys)], None))
    return {"L": L, "R": R, "alpha": alpha, "ystats": ys}


def _condition(native, c, Z, y, Xq, noise, option):
    c.set_option(native.OPT_HIDDEN_TAIL, option)
    try:
        c.gp_condition(y, Z=Z, noise=noise)
        st = _state_bytes(native, c)
        st["acq"] = c.acq_eval(Xq, float(y.min()), grad=False)
        seen = float(np.median(np.diag(np.tril(st["L"]) @ np.tril(st["L"]).T) - np.diag(c.gram())))
        st["rung"] = np.array(min(RUNGS, key=lambda r: abs(r - seen)))
    finally:
        c.set_option(native.OPT_HIDDEN_TAIL, 1)
    return st


def _assert_same(a, b, what):
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), (what, key, float(np.nanmax(np.abs(a[key] - b[key]))))


@pytest.mark.parametrize("n,k", SHAPES)
def test_folded_root_inverse_has_the_separate_launches_bytes(native, ctx, n, k):
    Z, y, Xq = _inputs(n, k)
    off = _condition(native, ctx, Z, y, Xq, 1e-4, 0)
    on = _condition(native, ctx, Z, y, Xq, 1e-4, 1)
    assert np.isfinite(off["R"]).all() and np.isfinite(off["acq"]).all()
    assert float(off["rung"]) == 0.0
    # R is a root inverse at all: R L = I to rounding (the comparison below is not two copies of nothing)
    assert np.abs(np.tril(off["R"]) @ np.tril(off["L"]) - np.eye(n)).max() < 1e-6
    _assert_same(off, on, (n, k))


def test_jitter_retry_takes_the_same_rung(native, ctx):
    """n = 130, noise 0, two points duplicated (eight copies each): rung 0 fails (tests/test_gpu_score_split.py::
    test_retry_case_needs_jitter shows it for the numpy restatement), the factorisation runs again with jitter - through the
    folded sequence when the option is on.  The separate launches decide the rung."""
    from test_gpu_score_split import retry_case
    Z, y, Xq = retry_case()
    off = _condition(native, ctx, Z, y, Xq[:8], 0.0, 0)
    on = _condition(native, ctx, Z, y, Xq[:8], 0.0, 1)
    assert float(off["rung"]) > 0.0, "the separate launches factored the retry case at rung 0: the retry was not exercised"
    _assert_same(off, on, "retry")


def test_batch_of_three_equals_three_single_contexts(native):
    """A batch keeps the separate launches, single contexts fold: run b of a 3-run batch at n = 129 equals its own context."""
    n, k = 129, 4
    cases = [_inputs(n, k, seed=b) for b in range(3)]
    bt = native.Batch(3, max_n=192, max_d=8, max_q=16)
    try:
        bt.gp_condition_begin(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), gp_noise=1e-4)
        _, status = bt.gp_wait_eval([c[2] for c in cases], [float(c[1].min()) for c in cases])
        assert (status == 0).all()
        for b, (Z, y, Xq) in enumerate(cases):
            in_batch = _state_bytes(native, bt.ctx[b])
            in_batch["acq"] = bt.ctx[b].acq_eval(Xq, float(y.min()), grad=False)
            single = native.Context(max_n=192, max_d=8, max_q=16)
            try:
                alone = _condition(native, single, Z, y, Xq, 1e-4, 1)
            finally:
                single.close()
            del alone["rung"]
            _assert_same(in_batch, alone, ("batch run", b))
    finally:
        bt.close()
