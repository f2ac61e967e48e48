"""The initial pick of a single run's one native call (pcabo_propose_acqf), on the CPU: botorch's initialize_q_batch as
pcabo.initializers runs it on torch's GLOBAL generator, against the native pick fed with `torch.get_rng_state()` - once in two
halves as the one call makes it (AheadPick of csrc/host_side.h, the helper pcabo_propose_acqf itself runs: what a draw can change
of the blob kept, the variates drawn before the scores are handed over, the pick from them - through pcabo_debug_boltzmann_two_halves,
also with a put-back and a second draw in between) and once through pcabo_boltzmann_pick_rows.  Equal indices, and the generator's
state after equal byte for byte.

The cases follow the rule by which pcabo.acqopt.optimize_acqf takes the native pick at all: fewer picks than values.  With as many
picks as values initialize_q_batch returns arange(n) and draws nothing; those cases are kept and asserted as such.  A row without
spread, or whose largest ratios tie (weights of 4e306 over a variate below 1 give several inf: met at eta = 2000, seed 3199; the
order torch's topk leaves ties in is its own), reports flag 1, leaves the blob as it was and the torch path decides, as in production.
5 632 seeds: 3 520 of them have fewer picks than values, and at least 3 000 of those must come back PICKED by the native code,
in all three ways (asserted).

The fourth door of the blob checker, pcabo_propose_acqf itself, needs a context: tests/test_gpu_propose.py.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

N_VALUES = (2, 3, 10, 512)
ERR_ARG = -1                       # PCABO_ERR_ARG
SEEDS = 5632                       # 704 seeds for each of the 4 sizes x 2 pick counts; 5 of the 8 have fewer picks than values
NATIVE_PICKS = 3000                # ... and at least this many of their 3 520 seeds must be PICKED natively (not handed to torch)


@pytest.fixture(scope="module")
def lib(native):
    from pcabo import hostrng as H
    assert H.native_ok()
    L = native.LIB
    L.pcabo_debug_boltzmann_two_halves.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                                    C.c_void_p]
    L.pcabo_debug_boltzmann_two_halves.restype = C.c_int
    return L


def two_halves(lib, blob, vals, n_pick, eta, put_back=0):
    out, flag = np.full(n_pick, -1, dtype=np.int64), C.c_int(-1)
    rc = lib.pcabo_debug_boltzmann_two_halves(blob.ctypes.data, vals.ctypes.data, len(vals), n_pick, eta, put_back, out.ctypes.data,
                                              C.byref(flag))
    return rc, out, flag.value


def two_halves_after_put_back(lib, blob, vals, n_pick, eta):
    """drawn, put back (the scores never came), drawn again and picked"""
    return two_halves(lib, blob, vals, n_pick, eta, put_back=1)


def pick_rows(lib, blob, vals, n_pick, eta):
    out, flag = np.full(n_pick, -1, dtype=np.int64), C.c_int(-1)
    ptr = (C.c_void_p * 1)(blob.ctypes.data)
    rc = lib.pcabo_boltzmann_pick_rows(ptr, vals.ctypes.data, 1, len(vals), n_pick, eta, out.ctypes.data, C.byref(flag))
    return rc, out, flag.value


def torch_pick(seed, vals, n_pick, eta):
    """(indices, global generator's state after) of pcabo.initializers.initialize_q_batch from torch.manual_seed(seed)"""
    from pcabo import initializers as I
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        idx = I.initialize_q_batch(vals, n_pick, eta)
    return np.asarray(idx), torch.get_rng_state().numpy().copy()


def case(seed):
    """Scores of seed's case: size, pick count, temperature, scale 1e-300 .. 1e300, and every third case ties."""
    rng = np.random.default_rng(seed)
    n = N_VALUES[seed % 4]
    n_pick = 1 if (seed // 4) % 2 == 0 else min(n, 10)
    # eta (n - 1) / sqrt(n) >= 700 is where botorch's halving loop can run at all: eta = 1 never reaches it
    eta = (1.0, 1.0, 40.0, 2000.0)[(seed // 8) % 4]
    scale = 10.0 ** rng.uniform(-300.0, 300.0) if (seed // 32) % 2 == 0 else 10.0 ** rng.uniform(-3.0, 2.0)
    vals = rng.normal(size=n) * scale + (rng.normal() * scale if seed % 5 else 0.0)
    kind = seed % 3
    if kind == 1 and n > 2:
        vals[rng.integers(0, n, size=max(2, n // 3))] = vals.max()          # ties in the maximum
    elif kind == 2 and n > 2:
        vals[:] = vals[rng.integers(0, max(2, n // 4), size=n)]             # repeated values everywhere
    return np.ascontiguousarray(vals), n_pick, eta


def test_two_halves_and_pick_rows_equal_torch_on_the_global_generator(lib):
    halved = flat = native_picks = 0
    for seed in range(SEEDS):
        vals, n_pick, eta = case(seed)
        n = len(vals)
        want, state = torch_pick(seed, vals, n_pick, eta)
        torch.manual_seed(seed)
        start = torch.get_rng_state().numpy().copy()
        if n_pick == n:                   # initialize_q_batch's own early return: every index, nothing drawn; never native
            assert np.array_equal(want, np.arange(n)) and np.array_equal(state, start), seed
            continue
        with np.errstate(all="ignore"):
            z = (vals - vals.mean()) / vals.std(ddof=1)
            halved += bool(np.isinf(np.exp(eta * z)).any())
        flags = set()
        for fn in (two_halves, pick_rows, two_halves_after_put_back):
            blob = start.copy()
            rc, got, flag = fn(lib, blob, vals, n_pick, eta)
            assert rc == 0 and flag in (0, 1), (seed, fn.__name__, rc, flag)
            flags.add(flag)
            if flag == 1:                 # no spread by the library's statistic: nothing drawn, torch's own reduction decides
                assert np.array_equal(blob, start), (seed, fn.__name__)
                flat += fn is two_halves
                torch.set_rng_state(torch.from_numpy(blob))
                from pcabo import initializers as I
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    got = np.asarray(I.initialize_q_batch(vals, n_pick, eta))
                blob = torch.get_rng_state().numpy()
            assert np.array_equal(got, want), (seed, fn.__name__, n, n_pick, eta, got, want)
            assert np.array_equal(blob, state), (seed, fn.__name__, "generator state")
        assert len(flags) == 1, (seed, flags)
        native_picks += flags == {0}
    assert halved >= 20, halved           # the halving loop did run
    assert flat < SEEDS // 8, flat        # ... and the flat path is the exception (scores that underflow to equal)
    assert native_picks >= NATIVE_PICKS, native_picks      # seeds whose indices and state came from the native pick, all three ways


def test_constant_scores_report_no_spread_and_leave_the_generator(lib):
    from pcabo import initializers as I
    for n, n_pick in ((2, 1), (10, 3), (512, 10)):
        vals = np.full(n, -7.5)
        torch.manual_seed(11 + n)
        start = torch.get_rng_state().numpy().copy()
        for fn in (two_halves, pick_rows, two_halves_after_put_back):
            blob = start.copy()
            rc, got, flag = fn(lib, blob, vals, n_pick, 1.0)
            assert (rc, flag) == (0, 1) and np.array_equal(blob, start), (n, fn.__name__)
            assert (got == -1).all()
        torch.manual_seed(11 + n)
        want = torch.randperm(n)[:n_pick].numpy()
        torch.manual_seed(11 + n)
        with pytest.warns(RuntimeWarning, match="are the same"):
            assert np.array_equal(I.initialize_q_batch(vals, n_pick), want)


def test_a_nan_score_reports_no_spread_and_torch_raises_as_before(lib):
    from pcabo import initializers as I
    rng = np.random.default_rng(3)
    for n, n_pick, at in ((3, 1, 0), (10, 3, 9), (512, 10, 100)):
        vals = rng.normal(size=n)
        vals[at] = np.nan
        torch.manual_seed(5)
        start = torch.get_rng_state().numpy().copy()
        for fn in (two_halves, pick_rows, two_halves_after_put_back):
            blob = start.copy()
            rc, _, flag = fn(lib, blob, vals, n_pick, 1.0)
            assert (rc, flag) == (0, 1) and np.array_equal(blob, start), (n, fn.__name__)
        with pytest.raises(RuntimeError):
            I.initialize_q_batch(vals, n_pick)


def test_a_blob_that_would_read_past_its_state_is_refused(lib, native):
    """left in [1, 624], and left == 1 or next + left <= 625; seeded.  (Layout: uint64 seed, int32 left, int32 seeded, uint64 next.)"""
    from pcabo import hostrng as H
    vals = np.ascontiguousarray(np.random.default_rng(1).normal(size=16))
    w = np.exp(vals)[None]
    good = torch.Generator().manual_seed(3).get_state().numpy().copy()

    def doors(blob):
        bits = np.empty(8, dtype=np.int64)
        out = np.zeros((1, 4), dtype=np.int64)
        ptr = (C.c_void_p * 1)(blob.ctypes.data)
        return (lib.pcabo_torch_randint2(blob.ctypes.data, 8, bits.ctypes.data),
                pick_rows(lib, blob, vals, 4, 1.0)[0],
                lib.pcabo_torch_multinomial_rows(ptr, w.ctypes.data, 1, 16, 4, out.ctypes.data),
                two_halves(lib, blob, vals, 4, 1.0)[0])

    def shaped(left, nxt, seeded=1):
        b = good.copy()
        b[8:12] = np.frombuffer(np.int32(left).tobytes(), dtype=np.uint8)
        b[12:16] = np.frombuffer(np.int32(seeded).tobytes(), dtype=np.uint8)
        b[16:24] = np.frombuffer(np.uint64(nxt).tobytes(), dtype=np.uint8)
        return b

    assert H.BLOB_BYTES == native.TORCH_BLOB_BYTES == good.nbytes
    for left, nxt in ((1, 0), (1, 624), (1, 10 ** 6), (624, 1), (2, 623), (300, 325)):
        assert doors(shaped(left, nxt)) == (0, 0, 0, 0), (left, nxt)
    wraps = ((300, 2 ** 64 - 299, 1), (2, 2 ** 64 - 1, 1), (624, 2 ** 64 - 623, 1), (300, 2 ** 63, 1))      # next + left wraps past 2^64
    assert doors(shaped(1, 2 ** 64 - 1)) == (0, 0, 0, 0)               # left == 1: the next draw refills, `next` is not read
    for left, nxt, seeded in ((624, 2, 1), (2, 624, 1), (300, 326, 1), (10, 624, 1), (0, 0, 1), (625, 0, 1), (-3, 0, 1), (300, 10, 0)) + wraps:
        assert doors(shaped(left, nxt, seeded)) == (ERR_ARG,) * 4, (left, nxt, seeded)
