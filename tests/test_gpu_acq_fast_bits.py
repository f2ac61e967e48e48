"""The single-run acquisition kernel k_acq_fast keeps its bits when its reductions change form.

k_acq_fast reduces many values per wave (the v rows of its slab, |v|^2 and mu_s, the gradient pair of each component).  They
went from one wave_sum per value to wave_sum_multi (pcabo_internal.h), which builds the same lane tree for N values at once.
The trajectory of a run depends on the last ulp of every evaluation, so the claim is checked bit for bit: the helper against
N calls of wave_sum, and the kernel against tests/golden/acq_fast_hashes.json, written by tools/gpu_acq_fast_hashes.py from
the build before the change."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lanes(rng, n, kind):
    if kind == "normal":
        return rng.normal(size=(n, 64))
    if kind == "wide":        # mixed signs, magnitudes 1e-300 .. 1e300: every tree shape rounds (or overflows) differently
        return rng.choice([-1.0, 1.0], (n, 64)) * 10.0 ** rng.uniform(-300, 300, (n, 64))
    if kind == "cancel":      # pairs that cancel exactly next to tiny values, signed zeros, subnormals
        x = rng.normal(size=(n, 64)) * 1e16
        x[:, 32:] = -x[:, :32]
        x[:, ::7] = rng.choice([0.0, -0.0, 5e-324, -5e-324, 1e-3], (n, len(range(0, 64, 7))))
        return x
    raise ValueError(kind)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 10, 13, 20, 33, 64])
def test_wave_sum_multi_equals_wave_sum_bit_for_bit(native, n):
    fn = native.LIB.pcabo_debug_wave_sum_multi
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(100 + n)
    for kind in ("normal", "wide", "cancel"):
        for _ in range(4):
            x = np.ascontiguousarray(_lanes(rng, n, kind))
            ref, multi, uni = np.empty(n), np.empty(n), np.empty(n)
            mism = np.zeros(n, dtype=np.int32)
            assert fn(x.ctypes.data, n, ref.ctypes.data, multi.ctypes.data, uni.ctypes.data, mism.ctypes.data) == 0
            assert ref.tobytes() == multi.tobytes(), (kind, ref, multi)
            assert ref.tobytes() == uni.tobytes(), (kind, ref, uni)
            assert not mism.any(), (kind, mism)      # every lane that holds a value holds the owner's bits


def test_acq_fast_bits_are_pinned(native):
    """Value + gradient of k_acq_fast, plain and resident, for every <SLAB, NB> instantiation and k in {3, 17, 36, 40}."""
    spec = importlib.util.spec_from_file_location("gpu_acq_fast_hashes", os.path.join(ROOT, "tools", "gpu_acq_fast_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "acq_fast_hashes.json")))["cases"]
    got = mod.compute()
    assert set(got) == set(golden)
    for case in golden:
        assert got[case] == golden[case], case
