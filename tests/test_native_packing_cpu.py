"""The binding's numpy-only helpers - pack_rows (one run's points per row of a batch call's buffer), per_run (one entry per run,
None or only the status for a run the call skipped) and fit_result (what a likelihood evaluation or a fit returns) - against the
inline code they replaced, which this file restates once: byte for byte, key order and Python types included.  No device."""
import math

import numpy as np
import pytest


# ---- the code as it stood inline in pcabo/_native.py (Batch.gp_wait_eval, gp_eval_begin, gp_extend, gp_loo, gp_fit ...) ----------
def inline_pack(blocks, B, row, buf=None, reuse=False):
    """Fresh buffer (gp_wait_eval, gp_posterior, _pack_ics, _pack_z; gp_extend skips None) or the kept one, where an entry that
    is a view of it is not copied (gp_eval_begin, acq_score_begin)."""
    if buf is None:
        buf = np.zeros((B, row))
    for b, xq in enumerate(blocks):
        if xq is None:
            continue
        if not (reuse and isinstance(xq, np.ndarray) and xq.base is buf):
            buf[b, : xq.size] = np.ascontiguousarray(xq, dtype=np.float64).ravel()
    return buf


def inline_fit_result(theta, loss, ard=False):
    if ard:
        rho = theta[2:]
        ls = {"lengthscales": np.where(rho > 20.0, rho, np.log1p(np.exp(np.minimum(rho, 20.0))))}
    else:
        rho = float(theta[2])
        ls = {"lengthscale": math.log1p(math.exp(rho)) if rho <= 20.0 else rho}
    return {**ls, "noise": float(theta[0]), "mean_constant": float(theta[1]), "loss": float(loss), "theta": theta.copy()}


def inline_loo(status, mean, total):
    return [None if status[b] != 0 else {"mean": mean[b].copy(), "lpd_sum": float(total[b])} for b in range(len(status))]


def inline_batch_fit(status, th, loss, info, ks):
    return [{**inline_fit_result(th[b, : 2 + k], loss[b], True), "iterations": int(info[b, 0]),
             "evaluations": int(info[b, 1]), "warnflag": int(info[b, 2]), "task": int(info[b, 3]), "status": 0}
            if status[b] == 0 else {"status": int(status[b])} for b, k in enumerate(ks)]


def same(a, b):
    """Equal to the byte: containers by structure and key order, arrays by dtype, shape and bytes, scalars by type and repr."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return repr(a) == repr(b)


@pytest.fixture(scope="module")
def blocks():
    """B = 3 runs of k = (1, 3, 5) in max_d = 5, q = 2 points each."""
    rng = np.random.default_rng(7)
    return [rng.standard_normal((2, k)) for k in (1, 3, 5)]


@pytest.mark.parametrize("q", [2, 1])
def test_fresh_buffer_equals_the_inline_packing(native, blocks, q):
    xs = [x[:q] for x in blocks]
    want = inline_pack(xs, 3, q * 5)
    got = native.pack_rows(xs, q * 5)
    assert same(got, want) and got.flags.c_contiguous
    assert same(native.pack_rows(xs, q * 5, np.zeros((3, q * 5))), want)      # (a zeroed buffer handed in: what Batch does)
    wide = native.pack_rows(xs, q * 5, np.zeros((4, q * 5)))                   # a list shorter than the buffer: the rest stays zero
    assert same(wide[:3], want) and not wide[3].any()


def test_a_none_entry_leaves_its_row_alone(native, blocks):
    xs = [blocks[0], None, blocks[2]]
    assert same(native.pack_rows(xs, 10), inline_pack(xs, 3, 10))
    stale = np.full((3, 10), 9.25)
    assert same(native.pack_rows(xs, 10, stale.copy()), inline_pack(xs, 3, 10, stale.copy()))
    assert (native.pack_rows(xs, 10, stale.copy())[1] == 9.25).all()


def test_strided_and_float32_inputs_are_converted_as_before(native):
    rng = np.random.default_rng(8)
    big = rng.standard_normal((4, 10))
    xs = [big[::2, ::2],                                             # non-contiguous, 2 x 5
          rng.standard_normal((2, 3)).astype(np.float32),           # float32: widened exactly
          np.asfortranarray(rng.standard_normal((2, 4)))]           # column-major: flattened row by row
    assert not xs[0].flags.c_contiguous and not xs[2].flags.c_contiguous
    assert same(native.pack_rows(xs, 10), inline_pack(xs, 3, 10))


def test_views_of_the_row_buffer_are_not_written(native):
    """The no-copy case of every iteration: the caller drew its points straight into the rows (Batch.raw_row_buffer)."""
    rng = np.random.default_rng(9)
    buf = rng.standard_normal((3, 10))
    views = [buf[b, : 2 * k].reshape(2, k) for b, k in enumerate((1, 3, 5))]
    before = buf.tobytes()
    buf.flags.writeable = False                                     # any write would raise
    assert native.pack_rows(views, 10, buf) is buf and buf.tobytes() == before
    buf.flags.writeable = True
    # mixed: one run's points come from elsewhere and are copied in, the views stay as they lie
    other = rng.standard_normal((2, 3))
    twin = buf.copy()
    twin_views = [twin[b, : 2 * k].reshape(2, k) for b, k in enumerate((1, 3, 5))]
    got = native.pack_rows([views[0], other, views[2]], 10, buf)
    want = inline_pack([twin_views[0], other, twin_views[2]], 3, 10, twin, reuse=True)
    assert got is buf and same(got, want)


def test_a_reused_buffer_keeps_the_stale_tail(native, blocks):
    rng = np.random.default_rng(10)
    stale = rng.standard_normal((3, 10))
    got = native.pack_rows(blocks, 10, stale.copy())
    assert same(got, inline_pack(blocks, 3, 10, stale.copy(), reuse=True))
    for b, k in enumerate((1, 3, 5)):
        assert same(got[b, 2 * k:], stale[b, 2 * k:]) and same(got[b, : 2 * k], blocks[b].ravel())


def test_per_run_gives_none_or_the_status_for_skipped_runs(native):
    rng = np.random.default_rng(11)
    status = np.array([0, -1, -2, 0], dtype=np.int32)
    mean, total = rng.standard_normal((4, 6)), rng.standard_normal(4)
    got = native.per_run(status, lambda b: {"mean": mean[b].copy(), "lpd_sum": float(total[b])})
    assert same(got, inline_loo(status, mean, total)) and got[1] is None and got[2] is None
    assert got[0]["mean"].base is None                              # a copy, no view of the call's buffer
    built = []
    only = native.per_run(status, lambda b: built.append(b) or {"status": 0}, status_only=True)
    assert same(only, [{"status": 0}, {"status": -1}, {"status": -2}, {"status": 0}]) and built == [0, 3]
    assert type(only[1]["status"]) is int


def test_fit_result_equals_the_inline_dicts(native):
    rng = np.random.default_rng(12)
    for ard, theta in ((False, np.array([0.01, 0.3, -1.5])), (False, np.array([0.01, 0.3, 25.0])),
                       (True, np.array([0.02, -0.1, -30.0, 0.0, 19.5, 20.5, 40.0]))):
        loss, g, info = np.float64(1.25), rng.standard_normal(theta.size), np.array([7, 9, 0, 2], dtype=np.int32)
        plain = native.fit_result(theta, loss, ard)
        assert same(plain, inline_fit_result(theta, loss, ard)) and plain["theta"] is not theta
        assert same(native.fit_result(theta, loss, ard, grad=g), {**inline_fit_result(theta, loss, ard), "grad": g})
        assert native.fit_result(theta, loss, ard, grad=g)["grad"] is g
        assert same(native.fit_result(theta, loss, ard, info=info),
                    {**inline_fit_result(theta, loss, ard), "iterations": 7, "evaluations": 9, "warnflag": 0, "task": 2})


def test_a_batch_fit_built_from_the_two_helpers_equals_the_inline_list(native):
    """Batch.gp_fit_ard's results as Batch._fit_call builds them, on a status array mixing 0, -1 and -2."""
    rng = np.random.default_rng(13)
    ks, status = [1, 3, 5, 2], np.array([0, -2, 0, -1], dtype=np.int32)
    th, loss = rng.standard_normal((4, 7)), rng.standard_normal(4)
    info = rng.integers(0, 50, (4, 4)).astype(np.int32)
    got = native.per_run(status, lambda b: {**native.fit_result(th[b, : 2 + ks[b]], loss[b], True, info=info[b]), "status": 0},
                         status_only=True)
    assert same(got, inline_batch_fit(status, th, loss, info, ks))
