"""pcabo_bbob_eval_many (k_bbob_eval_many, csrc/kernels_bbob.hip; DeviceObjectives.eval_many): m candidates per run in one launch,
each with the bytes pcabo_bbob_eval gives it alone - both kernels are one work-group function - and the lock-step batch that uses
it for its q candidates."""
import ctypes as C
import warnings

import numpy as np
import pytest

from pcabo.bbob import BBOBProblem
from pcabo.bbob_device import DeviceObjectives

pytestmark = pytest.mark.gpu

FIDS = (15, 20, 21, 24)


@pytest.mark.parametrize("d", [2, 5])
def test_three_candidates_are_three_single_calls(native, d):
    probs = [BBOBProblem(fid, inst, d) for fid in FIDS for inst in (0, 1)]
    dev = DeviceObjectives(probs)
    try:
        rng = np.random.default_rng([7, d])
        X = rng.uniform(-5.0, 5.0, (len(probs), 3, d))
        X[::2, 1, d - 1] = 5.0 + 1e-9                                   # one candidate of every other run outside the box
        X[1, 2] = probs[1].optimum.x
        one = [dev.evaluate(X[:, j]) for j in range(3)]                  # (before the staging buffers grow)
        f, raw, oob = dev.eval_many(X)
        again = [dev.evaluate(X[:, j]) for j in range(3)]                # (and after)
        assert f.shape == raw.shape == oob.shape == (len(probs), 3)
        for j in range(3):
            for got, a, b in zip((f[:, j], raw[:, j], oob[:, j]), one[j], again[j]):
                assert np.ascontiguousarray(got).tobytes() == a.tobytes() == b.tobytes(), j
        assert np.array_equal(oob[:, 1], np.arange(len(probs)) % 2 == 0) and not oob[:, 0].any() and not oob[:, 2].any()
        assert np.all(f[oob] == 1000.0) and np.all(raw[oob] == 1000.0) and np.all(np.isfinite(f))
        f1, raw1, oob1 = dev.eval_many(X[:, :1])                         # m = 1 is the single call
        assert f1[:, 0].tobytes() == one[0][0].tobytes() and raw1[:, 0].tobytes() == one[0][1].tobytes()
        assert np.array_equal(oob1[:, 0], one[0][2])
        # the C entry: m < 1 refused, oob may be NULL
        lib, vp = native.LIB, lambda a: a.ctypes.data_as(C.c_void_p)
        Xc, out = np.ascontiguousarray(X), np.empty((len(probs), 3))
        assert lib.pcabo_bbob_eval_many(dev._h, vp(Xc), 0, -5.0, 5.0, 1000.0, vp(out), None) == -1
        assert lib.pcabo_bbob_eval_many(dev._h, vp(Xc), -2, -5.0, 5.0, 1000.0, vp(out), None) == -1
        assert lib.pcabo_bbob_eval_many(dev._h, None, 3, -5.0, 5.0, 1000.0, vp(out), None) == -1
        assert lib.pcabo_bbob_eval_many(dev._h, vp(Xc), 3, -5.0, 5.0, 1000.0, None, None) == -1
        assert lib.pcabo_bbob_eval_many(None, vp(Xc), 3, -5.0, 5.0, 1000.0, vp(out), None) == -1
        assert lib.pcabo_bbob_eval_many(dev._h, vp(Xc), 3, -5.0, 5.0, 1000.0, vp(out), None) == 0
        assert out.tobytes() == raw.tobytes()
        with pytest.raises(ValueError):
            dev.eval_many(X[:, :, :-1])
    finally:
        dev.close()


def test_batch_with_device_objectives_and_q3(native, monkeypatch):
    monkeypatch.delenv("SMOKE_TEST", raising=False)
    from pcabo.batchrun import BatchedPCABO
    out = []
    for dev in (False, True):
        r = BatchedPCABO([BBOBProblem(15, i, 5) for i in range(3)], [15051 + i for i in range(3)], 13, 6, q=3, device_objective=dev)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            r.run()
        out.append(r)
    host, devr = out
    for b in range(3):
        assert len(devr.f_evals[b]) == len(devr.x_evals[b]) == 13 and devr.failed[b] is None
        # the first iteration's three candidates come from the same model: same points, values as close as the two objectives are
        assert np.array_equal(np.vstack(host.x_evals[b])[:9], np.vstack(devr.x_evals[b])[:9])
        fa, fb = np.array(host.f_evals[b])[:9], np.array(devr.f_evals[b])[:9]
        assert np.abs(fa - fb).max() <= 1e-10 * max(1.0, np.abs(fa).max())
        assert len(devr.problems[b].log) == devr.problems[b].evaluations
