"""pcabo_inverse_map of a single context runs on the host (csrc/host_side.h: inverse_map_host) from the pinned wPCA results; the
device kernel k_inverse_map stays for batches and behind PCABO_OPT_HIDDEN_TAIL = 0.  The two must agree byte for byte: the kernel's
loop `s += z[c] * comps[c][j]` is a chain of fused multiply-adds in ascending c (its disassembly: one v_fmac_f64 per term), the host
runs the same chain with fma.

One context computes x both ways from the same wPCA: option 1 = host, option 0 = k_inverse_map.  The components reach the library
only through a weighted PCA, so comps are the orthonormal rows it found (entries in [-1, 1]) and k cannot exceed d: a case of the
grid that asks for k > d runs at the k the library then fixes, min(k, d).  The host arithmetic at every (k, d) of the grid on
arbitrary components, zeros and signed zeros among them, is csrc/host_selftest.cpp::test_inverse_map_host (`make asan ubsan`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 7, 8, 9, 36, 40)            # the edges of the kernel's 8-way unroll
DS = (1, 40, 100)
N = 112                              # > every d: all d components exist


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(max_n=N, max_d=max(DS), max_q=16)
    yield c
    c.close()


def _both(native, ctx, z):
    out = []
    for opt in (1, 0):
        ctx.set_option(native.OPT_HIDDEN_TAIL, opt)
        out.append(ctx.inverse_map(z))
    ctx.set_option(native.OPT_HIDDEN_TAIL, 1)
    return out


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("k", KS)
def test_host_inverse_map_has_the_kernels_bytes(native, ctx, k, d):
    rng = np.random.default_rng([k, d, 77])
    X = rng.uniform(-5.0, 5.0, (N, d))
    res = ctx.wpca(X, f=rng.normal(size=N), n_components=k)
    kk = res["k"]
    assert kk == min(k, d)
    assert np.abs(res["components"]).max() <= 1.0
    for rep in range(50):
        z = rng.uniform(-1e3, 1e3, kk)
        host, dev = _both(native, ctx, z)
        assert host.tobytes() == dev.tobytes(), (k, d, rep, np.abs(host - dev).max())
    assert np.isfinite(host).all()


@pytest.mark.parametrize("k,d", [(9, 40), (36, 100)])
def test_zeros_and_signed_zeros(native, ctx, k, d):
    """z of exact zeros of both signs (alone and mixed with values), on data whose last third of the coordinates is constant:
    those coordinates have no variance, and what the components hold there is multiplied by the zeros like everything else."""
    rng = np.random.default_rng([k, d, 78])
    X = rng.uniform(-5.0, 5.0, (N, d))
    X[:, d - d // 3:] = 1.25
    kk = ctx.wpca(X, f=rng.normal(size=N), n_components=k)["k"]
    assert kk == k
    signed = np.where(np.arange(kk) % 2 == 0, 0.0, -0.0)
    mixed = rng.uniform(-1e3, 1e3, kk)
    mixed[::3] = -0.0
    mixed[1::3] = 0.0
    for z in (np.zeros(kk), -np.zeros(kk), signed, mixed):
        host, dev = _both(native, ctx, z)
        assert host.tobytes() == dev.tobytes(), (k, d, z[:4])
