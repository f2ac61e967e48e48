"""Context.optimize_acqf keeps its bits on every path through its round loop: one group without a helper thread, the free-running
pair of two groups, lock-step rounds through the resident kernel, three stepping threads, plain launches, and the restart-group
kernel (tools/gpu_optimize_hashes.py lists the shapes).  tests/golden/optimize_paths_hashes.json was written by that tool from the
library as it was before the host side of the call (helper threads, packing, the free-running pair) moved into host_side.h, and
is never regenerated for a change that is not meant to change arithmetic.

Whether a call with PCABO_OPT_RESIDENT = 1 really takes the resident kernel depends on the machine: the process must be alone on
the device with one context (presence_alone) and the kernel's first answer must come within a millisecond, else plain launches
take over for the next calls.  The bits must not depend on it.  That is exactly what is pinned here: the same hashes whichever
evaluator ran, resident = not resident, and every restart group equal to that group optimised alone."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gpu_optimize_hashes", os.path.join(ROOT, "tools", "gpu_optimize_hashes.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "optimize_paths_hashes.json")))["cases"]


def test_golden_file_lists_every_shape_and_mode():
    """No GPU: the golden file holds a cand / vals / info hash for every state, shape and mode of the tool, and nothing else."""
    assert set(GOLDEN) == {"n%d" % n for n in H.NS}
    for state in GOLDEN.values():
        assert set(state) == set(H.SHAPES)
        for shape, rec in state.items():
            assert set(rec) == set(H.modes_of(shape))
            assert all(set(d) == {"cand", "vals", "info"} and all(len(h) == 64 for h in d.values()) for d in rec.values())
    assert sorted(-(-nr // limit) for nr, limit in H.SHAPES.values()) == [1, 2, 3, 12, 16]   # the group counts the paths need


@pytest.fixture(scope="module", params=H.NS)
def state(native, request):
    ctx, box, ics, best_f = H.open_state(native, request.param)
    yield request.param, ctx, box, ics, best_f
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(H.SHAPES))
def test_every_path_of_the_call_has_the_pinned_bits(native, state, shape):
    n, ctx, box, ics, best_f = state
    nr, limit = H.SHAPES[shape]
    golden = GOLDEN["n%d" % n][shape]
    got = {}
    for mode in H.modes_of(shape):
        H.set_mode(native, ctx, mode)
        cand, vals, info = got[mode] = H.optimize(ctx, box, ics[:nr], best_f, limit)
        assert info.shape == (-(-nr // limit), 4)
        assert H.digest(cand, vals, info) == golden[mode], (n, shape, mode)
        for gi in (0, info.shape[0] - 1):                         # a group's result does not depend on the groups beside it
            q0, q1 = gi * limit, min(nr, (gi + 1) * limit)
            c1, v1, i1 = H.optimize(ctx, box, ics[q0:q1], best_f, limit)
            assert np.array_equal(c1, cand[q0:q1]) and np.array_equal(v1, vals[q0:q1]) and np.array_equal(i1[0], info[gi]), \
                (n, shape, mode, gi)
    H.set_mode(native, ctx, "resident")
    for a, b in zip(got["resident"], got["launches"]):            # bit for bit, whichever evaluator the rounds took
        assert np.array_equal(a, b), (n, shape)
    assert golden["resident"] == golden["launches"]
