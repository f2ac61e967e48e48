"""ctypes binding of libpcabo.so (C ABI declared in include/pcabo.h).

Thin by design: numpy arrays (or torch tensors' device pointers) go in as plain pointers + sizes,
every status code is turned into a Python exception, and nothing here computes.  If the shared
library is missing the import of this module fails loudly - there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import numpy as np

ABI_VERSION = 2
KERNEL_MATERN52, KERNEL_RBF = 0, 1
ACQ_LOG_EI, ACQ_PI, ACQ_UCB = 0, 1, 2
PTR_HOST, PTR_DEVICE = 0, 1
OPT_RESIDENT, OPT_BESTF_F32, OPT_GROUP_ACQ, OPT_DEVICE_LBFGSB = 0, 1, 2, 3
OPT_HIDDEN_TAIL = 5
POST_OBS_NOISE = 1                              # gp_posterior: variance / covariance of an observation (likelihood noise added)
EXTEND_BELIEVER = 1                             # gp_extend: every point takes the model's own mean there (PCABO_EXTEND_BELIEVER)
PROPOSE_NO_WAKE = 1                             # propose_acqf: the stepping helper sleeps until the optimiser needs it
TORCH_BLOB_BYTES = 5056                         # torch.get_rng_state(): the CPU generator's state, as propose_acqf takes it
POST_CENTRED = 2                                # gp_posterior_samples: the mean is not added (the centred process)
POST_MAX_SAMPLES = 1024                         # gp_posterior_samples: most samples of one call
FIT_THETA0 = (0.006737946999085467, 0.0, 0.0)   # GP fit: (noise, mean constant, raw lengthscale) of a freshly built model
FIT_TASK_NOT_PD = -2                            # gp_fit's `task` when a trial theta could not be factored even with jitter
PROFILE_GROUPS = ("wpca", "gram", "cholesky", "root_inverse_alpha", "acq_partial", "acq_large_batches")

# Hardware queues.  A Batch drives the GPU from several worker threads on separate HIP streams (its gangs): the runtime's
# default of 4 hardware queues per process makes streams share queues, and kernels that share a queue run one after the other
# (-15 % for a 30-run batch).  The HIP runtime reads GPU_MAX_HW_QUEUES when it initialises; this library does NOT touch the
# environment - main.py and tools/ set it before the first GPU call (bench.py and the tests take the environment's, shared
# GPU machines do not accept processes that raise it), and Batch() warns when it is missing or too small.
HW_QUEUES_ENV, HW_QUEUES_WANTED = "GPU_MAX_HW_QUEUES", 16


def hw_queues_advice(streams: int) -> Optional[str]:
    """None if the environment provides enough hardware queues for `streams` concurrent streams, else what to set."""
    try:
        have = int(os.environ.get(HW_QUEUES_ENV, "4"))
    except ValueError:
        have = 4
    if have >= streams:
        return None
    return (f"{HW_QUEUES_ENV}={os.environ.get(HW_QUEUES_ENV, 'unset (default 4)')}: {streams} streams of this batch will share "
            f"hardware queues and their kernels serialise; set {HW_QUEUES_ENV}={max(HW_QUEUES_WANTED, streams)} in the environment "
            "before the process makes its first GPU call")


_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lib", "libpcabo.so")

# The C ABI, declared once: function -> its parameters, one letter each (ARG_TYPES), and after ">" what it returns where that is
# no int.  include/pcabo.h is the authority; tests/test_abi_and_host.py parses it and holds every entry here to it, kind by kind.
# The typed pointers (I, D, L, V) stand where callers pass C.byref(...) or a ctypes array; everything numpy hands over as an
# address is a plain "v" (_ptr).  A new C function gets its prototype in the header and one entry here.
FG_CALLBACK = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
ARG_TYPES = {
    "i": C.c_int, "d": C.c_double, "z": C.c_size_t, "l": C.c_int64, "q": C.c_longlong, "v": C.c_void_p, "s": C.c_char_p,
    "I": C.POINTER(C.c_int), "D": C.POINTER(C.c_double), "L": C.POINTER(C.c_int64), "V": C.POINTER(C.c_void_p), "f": FG_CALLBACK,
}
SIGNATURES = {
    "pcabo_abi_version": "", "pcabo_device_count": "", "pcabo_ctx_create": "iiiiV", "pcabo_ctx_destroy": "v",
    "pcabo_set_pointer_mode": "vi", "pcabo_set_option": "vii", "pcabo_last_error": "vsi", "pcabo_wpca": "vvvviiidivvvvvIv",
    "pcabo_gp_condition": "vvviivddi", "pcabo_gp_condition_begin": "vvviivddi", "pcabo_gp_condition_end": "v",
    "pcabo_gp_condition_end_eval": "vvidiiv", "pcabo_wpca_gp_condition_begin": "vvvviiidivvddivvvvI",
    "pcabo_wpca_results": "vvvvvI", "pcabo_gp_mll": "vvviivivDv", "pcabo_gp_fit": "vvviivivDv",
    "pcabo_gp_mll_ard": "vvviivivDv", "pcabo_gp_fit_ard": "vvviivivDv", "pcabo_acq_bounds": "vv", "pcabo_acq_eval": "vvidiivv",
    "pcabo_logei": "vvidivv", "pcabo_gp_posterior": "vviivvv", "pcabo_batch_gp_posterior": "vviivvvv",
    "pcabo_gp_posterior_sample": "vviivivvD", "pcabo_batch_gp_posterior_sample": "vviivivvvv", "pcabo_gp_loo": "vvvvvD",
    "pcabo_batch_gp_loo": "vvvvvvv", "pcabo_gp_extend": "vvvii", "pcabo_gp_truncate": "vi", "pcabo_gp_extended": "vII",
    "pcabo_batch_gp_extend": "vvviiv", "pcabo_batch_gp_truncate": "viv", "pcabo_batch_gp_extended": "vII",
    "pcabo_optimize_acqf": "vviividiivvvI", "pcabo_propose_acqf": "vvivdiividiiivvvvvvIIv", "pcabo_inverse_map": "vvv",
    "pcabo_get_gp_state": "vvvvvv", "pcabo_get_gram": "vv", "pcabo_lbfgsb_minimize": "ivvvfviddiiiDIII",
    "pcabo_lbfgsb_set_vector_kernels": "i", "pcabo_lbfgsb_set_sum_order": "i", "pcabo_sobol_scramble": "vvi",
    "pcabo_sobol_draw": "vviivvv", "pcabo_sobol_draw_rows": "vvviivlv", "pcabo_torch_randint2": "vlv",
    "pcabo_torch_multinomial_rows": "vviiiv", "pcabo_boltzmann_pick_rows": "vviiidvv", "pcabo_set_profiling": "vi",
    "pcabo_get_profile": "viDLDD", "pcabo_get_profile_calibration": "vDD", "pcabo_reset_profile": "v",
    "pcabo_batch_create": "iiiiiV", "pcabo_batch_destroy": "v", "pcabo_batch_last_error": "vsi", "pcabo_batch_ctx": "vi>v",
    "pcabo_batch_wpca_gp_condition_begin": "vvvvviiididdi", "pcabo_batch_wpca_results": "vvvvvv",
    "pcabo_batch_acq_bounds": "vv", "pcabo_batch_acq_score": "vviviivv", "pcabo_batch_acq_score_begin": "vvivii",
    "pcabo_batch_acq_score_end": "vivv", "pcabo_batch_gp_condition_end_eval": "vviviivv",
    "pcabo_batch_optimize_acqf": "vviiviviivvvvv", "pcabo_batch_inverse_map": "vvv", "pcabo_batch_device_acq_eval": "vviviivv",
    "pcabo_batch_busy": "v", "pcabo_batch_gp_condition_end_eval_begin": "vvivii",
    "pcabo_batch_gp_condition_end_eval_end": "vviviivv", "pcabo_batch_optimize_acqf_begin": "vviivivii",
    "pcabo_batch_optimize_acqf_end": "viivvvvv", "pcabo_batch_inverse_map_begin": "vv", "pcabo_batch_inverse_map_end": "vv",
    "pcabo_batch_set_input_strides": "vzzz", "pcabo_batch_gp_condition_begin": "vvviivddi", "pcabo_batch_gp_mll": "vvvvv",
    "pcabo_batch_gp_fit": "vvvvv", "pcabo_batch_gp_fit_rounds": "v", "pcabo_batch_gp_mll_ard": "vvivvv",
    "pcabo_batch_gp_fit_ard": "vvivvv", "pcabo_batch_set_profiling": "vi", "pcabo_batch_get_profile": "vv",
    "pcabo_batch_set_active": "vv", "pcabo_batch_set_workers": "vi", "pcabo_batch_set_option": "vii",
    "pcabo_device_lbfgsb_limits": "III", "pcabo_bbob_table_doubles": "i", "pcabo_bbob_create": "iiivvV",
    "pcabo_bbob_destroy": "v", "pcabo_bbob_eval": "vvdddvv", "pcabo_bbob_eval_many": "vvidddvv", "pcabo_comm_unique_id": "s",
    "pcabo_comm_create": "siiiV", "pcabo_gather_best": "vviv", "pcabo_comm_last_error": "vsi", "pcabo_comm_destroy": "v",
}
EXPORTS = list(SIGNATURES)
# debug exports (not in include/pcabo.h): the branch counters of the host L-BFGS-B and what the device optimiser writes per group.
# Declared where the library has them (the host-only checker builds of the library have no batch).
DEBUG_SIGNATURES = {
    "pcabo_debug_lbfgsb_branch_names": "si", "pcabo_debug_lbfgsb_branches": "vi",
    "pcabo_debug_batch_lbfgsb_branches": "vvi", "pcabo_debug_batch_lbfgsb_device_out": "vvi",
}


class PcaboError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libpcabo error {code}: {msg}")
        self.code = code


def lib_path() -> str:
    # PCABO_LIB selects another build of the SAME library (diagnostic builds such as libpcabo_timing.so)
    return os.path.normpath(os.environ.get("PCABO_LIB") or _LIB_PATH)


def _declare(lib, table, optional=False) -> None:
    for name, code in table.items():
        if optional and not hasattr(lib, name):
            continue
        args, _, ret = code.partition(">")
        fn = getattr(lib, name)
        fn.argtypes = [ARG_TYPES[c] for c in args]
        fn.restype = ARG_TYPES[ret or "i"]


def _load() -> C.CDLL:
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C para-ortho-pca-bo_amd/csrc`).  There is no CPU fallback for the HIP path.")
    lib = C.CDLL(path)
    lib.pcabo_abi_version.restype = C.c_int
    if lib.pcabo_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: ABI version mismatch")
    _declare(lib, SIGNATURES)
    _declare(lib, DEBUG_SIGNATURES, optional=True)
    return lib


LIB = _load()


def _branch_names():
    buf = C.create_string_buffer(2048)
    count = LIB.pcabo_debug_lbfgsb_branch_names(buf, 2048)
    names = tuple(buf.value.decode().split(","))
    assert len(names) == count
    return names


LBFGSB_BRANCHES = _branch_names()               # the counters' names, in the order of the enum in csrc/lbfgsb.h
DEVICE_GROUP_FIELDS = ("niter", "nfev", "warnflag", "task", "status", "evaluations", "ties", "evaluation_cap")


def device_count() -> int:
    return int(LIB.pcabo_device_count())


def device_lbfgsb_limits():
    """(max n, max k, max points per restart group) of the device-resident optimiser (pcabo_device_lbfgsb_limits; host code)."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    LIB.pcabo_device_lbfgsb_limits(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _ptr(a: Optional[np.ndarray]):
    # (the address as an int - ctypes converts it for a c_void_p parameter; half the cost of data_as(), and a lock-step
    # iteration of 30 runs hands ~180 arrays to the library.  The caller keeps `a` alive across the call.)
    return None if a is None else a.ctypes.data


def _f64(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def sample_base(q: int, n_samples=None, base_samples=None, seed=None) -> np.ndarray:
    """The S x q base samples of a gp_posterior_samples call: the caller's `base_samples`, or `n_samples` standard normal rows from
    np.random.default_rng(seed) - a generator of its own, so neither numpy's global state nor torch's moves (a run's trajectory
    depends on both).  Exactly one of the two is given (ValueError otherwise, and for a base that is not S x q)."""
    if (n_samples is None) == (base_samples is None):
        raise ValueError("give exactly one of n_samples and base_samples")
    if base_samples is not None:
        if seed is not None:
            raise ValueError("seed goes with n_samples: base_samples are the draw")
        base = np.ascontiguousarray(base_samples, dtype=np.float64)
        if base.ndim != 2 or base.shape[1] != q or base.shape[0] < 1:
            raise ValueError(f"base_samples must be S x q = S x {q}, got {base.shape}")
        return base
    S = int(n_samples)
    if S < 1:
        raise ValueError("n_samples must be at least 1")
    return np.random.default_rng(seed).standard_normal((S, q))


def pack_rows(blocks, row: int, out: Optional[np.ndarray] = None) -> np.ndarray:
    """The (B, row) buffer the batch calls take one run's points per row in: blocks[b], flattened, at the head of row b.  `out`
    None: a fresh zeroed buffer of len(blocks) rows; else rows are written in place and whatever lies behind a block stays (the
    library reads only the head).  A block that is a view of `out` already lies in its row (Batch.raw_row_buffer) and is not
    copied; a None block's row is left alone.  The blocks are numpy arrays of any layout and dtype."""
    kept, asarray, f64 = out is not None, np.asarray, np.float64            # (locals: this loop runs B times per call of an iteration)
    if not kept:
        out = np.zeros((len(blocks), row))
    for b, x in enumerate(blocks):
        if x is None or (kept and x.base is out):
            continue
        out[b, : x.size] = asarray(x, f64).ravel()                          # (row by row, whatever x's layout)
    return out


def per_run(status, build, status_only: bool = False) -> list:
    """One entry per run of a batch call: build(b) where status[b] == 0; for a run the call skipped None, or {"status": code}."""
    return [build(b) if status[b] == 0 else ({"status": int(status[b])} if status_only else None) for b in range(len(status))]


def fit_result(theta, loss, ard=False, grad=None, info=None) -> dict:
    """What a likelihood evaluation (`grad`) or a fit (`info`: iterations, evaluations, warnflag, task) returns for one model at
    theta = (noise, mean constant, raw lengthscale | rho_1 .. rho_k)."""
    if ard:                                             # softplus as torch (and the library) compute it
        rho = theta[2:]
        out = {"lengthscales": np.where(rho > 20.0, rho, np.log1p(np.exp(np.minimum(rho, 20.0))))}
    else:
        rho = float(theta[2])
        out = {"lengthscale": math.log1p(math.exp(rho)) if rho <= 20.0 else rho}
    out.update(noise=float(theta[0]), mean_constant=float(theta[1]), loss=float(loss), theta=theta.copy())
    if grad is not None:
        out["grad"] = grad
    if info is not None:
        out.update(iterations=int(info[0]), evaluations=int(info[1]), warnflag=int(info[2]), task=int(info[3]))
    return out


class _Handle:
    """An object of the library behind one handle: its error text, the check of a status code, its end, and a failed creation."""
    _last_error = _destroy = None                       # the library's functions for this kind of handle
    _NOT_CREATED = "no usable HIP device (the HIP path has no CPU fallback)"

    def _create(self, create, *args) -> None:
        self._h = C.c_void_p()
        rc = create(*args, C.byref(self._h))
        if rc != 0:                                     # (the library may hand back a half-made object that holds the message)
            msg = self._err() if self._h else self._NOT_CREATED
            _Handle.close(self)
            raise PcaboError(rc, msg)

    def _err(self) -> str:
        if self._last_error is None:
            return self._NOT_CREATED
        buf = C.create_string_buffer(512)
        self._last_error(self._h, buf, 512)
        return buf.value.decode(errors="replace")

    def _chk(self, rc: int) -> None:
        if rc != 0:
            raise PcaboError(rc, self._err())

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(_Handle):
    """One per-run device context (a HIP stream + workspaces).  Not thread-safe; use one per thread."""
    _last_error, _destroy = LIB.pcabo_last_error, LIB.pcabo_ctx_destroy

    def __init__(self, max_n: int, max_d: int, max_q: int = 512, device: int = 0):
        self._create(LIB.pcabo_ctx_create, int(device), int(max_n), int(max_d), int(max_q))
        self.max_n, self.max_d, self.max_q, self.device = max_n, max_d, max_q, device
        self.n = self.d = self.k = 0

    def set_option(self, option: int, value: int) -> None:
        self._chk(LIB.pcabo_set_option(self._h, int(option), int(value)))

    def match_best_f_dtype(self, best_f) -> None:
        """botorch stores `torch.as_tensor(best_f)`: float32 for a Python float (or int), float64 for a numpy float64
        scalar (what a callable objective may return).  Tell the library which of the two the caller's value is."""
        f32 = 0 if isinstance(best_f, np.floating) and best_f.dtype == np.float64 else 1
        if getattr(self, "_bestf_f32", 1) != f32:
            self.set_option(OPT_BESTF_F32, f32)
            self._bestf_f32 = f32

    # ---- rows A-C -----------------------------------------------------------------------------
    def wpca(self, X, f=None, ranks=None, maximize=False, var_threshold=0.95, n_components=0, noise=None,
             want_Z=True, want_full=True):
        X = _f64(X)
        n, d = X.shape
        f_a = None if f is None else _f64(f, (n,))
        r_a = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.int64).reshape(n)
        nz = None if noise is None else _f64(noise, (n, d))
        rc_ = min(n, d)
        data_mean, pca_mean = np.empty(d), np.empty(d)
        comps = np.empty((rc_, d)) if want_full else None
        evr = np.empty(rc_) if want_full else None
        k = C.c_int(0)
        Z = np.empty((n, d)) if want_Z else None
        self._chk(LIB.pcabo_wpca(self._h, _ptr(X), _ptr(f_a), _ptr(r_a), n, d, int(bool(maximize)),
                                 float(var_threshold), int(n_components), _ptr(nz), _ptr(data_mean), _ptr(pca_mean),
                                 _ptr(comps), _ptr(evr), C.byref(k), _ptr(Z)))
        self.n, self.d, self.k = n, d, k.value
        if want_Z:
            Z = Z.reshape(-1)[: n * k.value].reshape(n, k.value).copy()
        return {"data_mean": data_mean, "pca_mean": pca_mean, "components": comps, "evr": evr, "k": k.value, "Z": Z}

    # ---- rows A-H in one enqueue -------------------------------------------------------------
    def wpca_gp_condition(self, X, y, f=None, ranks=None, maximize=False, var_threshold=0.95, n_components=0,
                          noise=None, lengthscale=0.6931471805599453, gp_noise=0.006737946999085467,
                          kernel=KERNEL_MATERN52, collect=True):
        """wpca(...) + gp_condition(y, wait=False) without the host round trip between them: returns the wPCA results
        while the conditioning is still running; call gp_wait() before using the GP.  collect=False only enqueues
        (returns None); wpca_results() then waits for the wPCA and returns its results."""
        X = _f64(X)
        n, d = X.shape
        y = _f64(y, (n,))
        f_a = None if f is None else _f64(f, (n,))
        r_a = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.int64).reshape(n)
        nz = None if noise is None else _f64(noise, (n, d))
        self._chk(LIB.pcabo_wpca_gp_condition_begin(
            self._h, _ptr(X), _ptr(f_a), _ptr(r_a), n, d, int(bool(maximize)), float(var_threshold),
            int(n_components), _ptr(nz), _ptr(y), float(lengthscale), float(gp_noise), int(kernel), None, None, None, None,
            None))
        self.n, self.d = n, d
        return self.wpca_results() if collect else None

    def wpca_results(self):
        n, d = self.n, self.d
        rc_ = min(n, d)
        data_mean, pca_mean, comps, evr = np.empty(d), np.empty(d), np.empty((rc_, d)), np.empty(rc_)
        k = C.c_int(0)
        self._chk(LIB.pcabo_wpca_results(self._h, _ptr(data_mean), _ptr(pca_mean), _ptr(comps), _ptr(evr), C.byref(k)))
        self.k = k.value
        return {"data_mean": data_mean, "pca_mean": pca_mean, "components": comps, "evr": evr, "k": k.value, "Z": None}

    # ---- rows D-H -----------------------------------------------------------------------------
    def gp_condition(self, y, Z=None, norm_bounds=None, lengthscale=0.6931471805599453,
                     noise=0.006737946999085467, kernel=KERNEL_MATERN52, wait=True):
        """wait=False enqueues the conditioning and returns; call gp_wait() before using the GP."""
        y = _f64(y).reshape(-1)
        n = y.shape[0]
        if Z is not None:
            Z = _f64(Z)
            k = Z.shape[1]
        else:
            k = self.k
        nb = None if norm_bounds is None else _f64(norm_bounds, (2, k))
        self._keep = (y, Z, nb)      # host buffers must outlive the asynchronous copies
        fn = LIB.pcabo_gp_condition if wait else LIB.pcabo_gp_condition_begin
        self._chk(fn(self._h, _ptr(Z), _ptr(y), n, k, _ptr(nb), float(lengthscale), float(noise), int(kernel)))
        self.n, self.k = n, k

    # ---- opt-in GP hyperparameter fit (pcabo_gp_mll / pcabo_gp_fit) ----------------------------
    def _fit_args(self, y, Z, norm_bounds):
        y = _f64(y).reshape(-1)
        Z = None if Z is None else _f64(Z)
        k = self.k if Z is None else Z.shape[1]
        nb = None if norm_bounds is None else _f64(norm_bounds, (2, k))
        return y, Z, k, nb

    @staticmethod
    def _theta(theta, k, ard):
        if not ard:
            return _f64(theta, (3,)).copy()
        if theta is None:                               # a freshly built model: (noise, mean constant, rho_1 .. rho_k = 0)
            return np.array(FIT_THETA0[:2] + (0.0,) * k, dtype=np.float64)
        return _f64(theta, (2 + k,)).copy()

    def _gp_mll(self, ard, y, theta, Z, norm_bounds, kernel):
        y, Z, k, nb = self._fit_args(y, Z, norm_bounds)
        th = self._theta(theta, k, ard)
        loss, g = C.c_double(0.0), np.empty(th.shape[0])
        fn = LIB.pcabo_gp_mll_ard if ard else LIB.pcabo_gp_mll
        self._chk(fn(self._h, _ptr(Z), _ptr(y), y.shape[0], k, _ptr(nb), int(kernel), _ptr(th), C.byref(loss), _ptr(g)))
        self.n, self.k = y.shape[0], k
        return fit_result(th, loss.value, ard, grad=g)

    def _gp_fit(self, ard, y, theta0, Z, norm_bounds, kernel):
        y, Z, k, nb = self._fit_args(y, Z, norm_bounds)
        th = self._theta(theta0, k, ard)
        loss, info = C.c_double(0.0), np.zeros(4, dtype=np.int32)
        fn = LIB.pcabo_gp_fit_ard if ard else LIB.pcabo_gp_fit
        self._chk(fn(self._h, _ptr(Z), _ptr(y), y.shape[0], k, _ptr(nb), int(kernel), _ptr(th), C.byref(loss), _ptr(info)))
        self.n, self.k = y.shape[0], k
        return fit_result(th, loss.value, ard, info=info)

    def gp_mll(self, y, theta=FIT_THETA0, Z=None, norm_bounds=None, kernel=KERNEL_MATERN52):
        """Loss of the GP fit and its gradient at theta = (noise, mean constant, raw lengthscale); the context is left
        conditioned at theta.  Returns the fit's dict (`lengthscale`, `noise`, `mean_constant`, `loss`) with `grad` (3,)."""
        return self._gp_mll(False, y, theta, Z, norm_bounds, kernel)

    def gp_fit(self, y, theta0=FIT_THETA0, Z=None, norm_bounds=None, kernel=KERNEL_MATERN52):
        """Fit (noise, mean constant, raw lengthscale) by the marginal likelihood from theta0 (default: the model's initial
        values); the context is left conditioned at the fit.  Returns `lengthscale`, `noise`, `mean_constant`, `loss`,
        `iterations`, `evaluations`, `warnflag` (scipy's), `task` and `theta`."""
        return self._gp_fit(False, y, theta0, Z, norm_bounds, kernel)

    # ---- the same fit with one lengthscale per input (pcabo_gp_mll_ard / pcabo_gp_fit_ard) ------
    def gp_mll_ard(self, y, theta, Z=None, norm_bounds=None, kernel=KERNEL_MATERN52):
        """Loss of the ARD fit and its gradient at theta = (noise, mean constant, rho_1 .. rho_k), lengthscale_c =
        softplus(rho_c); the context is left conditioned at theta (the lengthscales folded into the Normalize ranges, which
        gp_state() then reports).  Returns `lengthscales` (k,), `noise`, `mean_constant`, `loss`, `theta` and `grad` (2 + k,)."""
        return self._gp_mll(True, y, theta, Z, norm_bounds, kernel)

    def gp_fit_ard(self, y, theta0=None, Z=None, norm_bounds=None, kernel=KERNEL_MATERN52):
        """gp_fit with one lengthscale per input, from theta0 (default: the model's initial values, every rho_c = 0).  Returns
        `theta`, `noise`, `mean_constant`, `lengthscales` (k,), `loss`, `iterations`, `evaluations`, `warnflag`, `task`; the
        context is left conditioned at the fit.  The fit keeps every rho_c >= ln 2^-40 = -27.73 (an optimiser bound like the
        noise's 1e-4; a start below it is clipped to it)."""
        return self._gp_fit(True, y, theta0, Z, norm_bounds, kernel)

    def gp_wait(self) -> None:
        self._chk(LIB.pcabo_gp_condition_end(self._h))
        self._keep = None

    def gp_wait_eval(self, Xq, best_f, maximize=False, acq=ACQ_LOG_EI) -> np.ndarray:
        """gp_wait() + acq_eval(Xq, grad=False) with the evaluation enqueued behind the conditioning (`best_f`: see acq_eval)."""
        Xq = _f64(Xq).reshape(-1, self.k)
        q = Xq.shape[0]
        val = np.empty(q)
        self._chk(LIB.pcabo_gp_condition_end_eval(self._h, _ptr(Xq), q, float(best_f), int(bool(maximize)), int(acq),
                                                  _ptr(val)))
        self._keep = None
        return val

    def acq_bounds(self) -> np.ndarray:
        b = np.empty((2, self.k))
        self._chk(LIB.pcabo_acq_bounds(self._h, _ptr(b)))
        return b

    # ---- row I --------------------------------------------------------------------------------
    def acq_eval(self, Xq, best_f, maximize=False, acq=ACQ_LOG_EI, grad=True):
        """Acquisition values (and gradients) at Xq.  `best_f`: the acquisition's scalar - the incumbent for ACQ_LOG_EI and ACQ_PI;
        for ACQ_UCB, which has no incumbent, the slot carries kappa = sqrt(beta) (finite, >= 0; include/pcabo.h)."""
        Xq = _f64(Xq).reshape(-1, self.k)
        q = Xq.shape[0]
        val = np.empty(q)
        g = np.empty((q, self.k)) if grad else None
        self._chk(LIB.pcabo_acq_eval(self._h, _ptr(Xq), q, float(best_f), int(bool(maximize)), int(acq), _ptr(val),
                                     _ptr(g)))
        return (val, g) if grad else val

    # ---- posterior queries (pcabo_gp_posterior) -------------------------------------------------
    def gp_posterior(self, Xq, observation_noise=False, covariance=False) -> dict:
        """What the conditioned GP predicts at Xq (q x k, reduced space): {"mean" (q,), "variance" (q,), floored at 1e-10 as
        gpytorch's[, "covariance" (q, q), not floored]}; observation_noise adds the likelihood noise (include/pcabo.h)."""
        Xq = _f64(Xq).reshape(-1, self.k)
        q = Xq.shape[0]
        mean, var = np.empty(q), np.empty(q)
        cov = np.empty((q, q)) if covariance else None
        self._chk(LIB.pcabo_gp_posterior(self._h, _ptr(Xq), q, POST_OBS_NOISE if observation_noise else 0, _ptr(mean), _ptr(var),
                                         _ptr(cov)))
        out = {"mean": mean, "variance": var}
        if covariance:
            out["covariance"] = cov
        return out

    # ---- posterior samples (pcabo_gp_posterior_sample) -------------------------------------------
    def gp_posterior_samples(self, Xq, n_samples=None, base_samples=None, seed=None, observation_noise=False, centred=False) -> dict:
        """Joint draws of the conditioned GP at Xq (q x k, reduced space): {"samples" (S, q) = mean + base Lc^T, "mean" (q,), "jitter":
        the rung of 0, 1e-8, 1e-7, 1e-6 (relative to y_std^2) the covariance's Cholesky Lc needed}.  The base is `base_samples` (S x q)
        or n_samples rows from sample_base's own generator; centred leaves the mean out of the samples (include/pcabo.h)."""
        Xq = _f64(Xq).reshape(-1, self.k)
        q = Xq.shape[0]
        base = sample_base(q, n_samples, base_samples, seed)
        S = base.shape[0]
        samples, mean = np.empty((S, q)), np.empty(q)
        jitter = C.c_double(0.0)
        flags = (POST_OBS_NOISE if observation_noise else 0) | (POST_CENTRED if centred else 0)
        self._chk(LIB.pcabo_gp_posterior_sample(self._h, _ptr(Xq), q, flags, _ptr(base), S, _ptr(samples), _ptr(mean),
                                                C.byref(jitter)))
        return {"samples": samples, "mean": mean, "jitter": float(jitter.value)}

    # ---- leave-one-out predictions (pcabo_gp_loo) -------------------------------------------------
    def gp_loo(self) -> dict:
        """What the conditioned GP says about each of its n points from the other n - 1: {"mean" (n,), "variance" (n,) of the
        observation, "z" (n,) standardised residuals, "lpd" (n,) log predictive densities, "lpd_sum"}; hyperparameters and
        transforms are those of the full data (include/pcabo.h)."""
        n = self.n
        mean, var, z, lpd = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
        total = C.c_double(0.0)
        self._chk(LIB.pcabo_gp_loo(self._h, _ptr(mean), _ptr(var), _ptr(z), _ptr(lpd), C.byref(total)))
        return {"mean": mean, "variance": var, "z": z, "lpd": lpd, "lpd_sum": float(total.value)}

    # ---- appending points and taking them back (pcabo_gp_extend / pcabo_gp_truncate) -----------------
    def gp_extend(self, Zp, y=None) -> int:
        """Append the points Zp (p x k, reduced space) with values y to the conditioned GP, one after the other, transforms and
        hyperparameters held (botorch's condition_on_observations); y=None is believer mode: every point takes the model's own
        mean there.  All or nothing (PcaboError -2 leaves the context as it was).  Returns the new n (include/pcabo.h)."""
        Zp = _f64(Zp).reshape(-1, self.k)
        p = Zp.shape[0]
        yv = None if y is None else _f64(y, (p,))
        self._chk(LIB.pcabo_gp_extend(self._h, _ptr(Zp), _ptr(yv), p, EXTEND_BELIEVER if y is None else 0))
        self.n += p
        return self.n

    def gp_truncate(self, n0=None) -> int:
        """Take back the appended points from n0 on (None: all of them, back to n_base).  Returns the new n."""
        n0 = self.n_base if n0 is None else int(n0)
        self._chk(LIB.pcabo_gp_truncate(self._h, n0))
        self.n = n0
        return self.n

    @property
    def n_base(self) -> int:
        """The n of the last conditioning or fit: gp_extend appends behind it."""
        nb, n = C.c_int(0), C.c_int(0)
        self._chk(LIB.pcabo_gp_extended(self._h, C.byref(nb), C.byref(n)))
        return int(nb.value)

    # ---- rows M-N -----------------------------------------------------------------------------
    def optimize_acqf(self, ics, bounds, best_f, maximize=False, acq=ACQ_LOG_EI, batch_limit=5, maxiter=200):
        """Multi-start L-BFGS-B from `ics` inside `bounds`; `best_f` as in acq_eval (ACQ_UCB: kappa).  Returns (candidates, values,
        per-group (iterations, evaluations, warnflag, task), botorch's retry flag)."""
        ics = _f64(ics).reshape(-1, self.k)
        nr = ics.shape[0]
        bounds = _f64(bounds, (2, self.k))
        cand = np.empty((nr, self.k))
        vals = np.empty(nr)
        ng = (nr + batch_limit - 1) // batch_limit
        info = np.zeros((ng, 4), dtype=np.int32)
        failed = C.c_int(0)
        self._chk(LIB.pcabo_optimize_acqf(self._h, _ptr(ics), nr, int(batch_limit), _ptr(bounds), int(maxiter),
                                          float(best_f), int(bool(maximize)), int(acq), _ptr(cand), _ptr(vals),
                                          _ptr(info), C.byref(failed)))
        return cand, vals, info, bool(failed.value)

    def propose_acqf(self, raw, blob, num_restarts, bounds, best_f, maximize=False, acq=ACQ_LOG_EI, batch_limit=5, maxiter=200,
                     eta=1.0, wake=True) -> dict:
        """gp_wait_eval / acq_eval(grad=False) of the raw samples, botorch's initialize_q_batch(eta) and optimize_acqf in one
        call (pcabo_propose_acqf).  `blob`: the state of torch's CPU generator as a contiguous uint8 array of 5056 bytes
        (`torch.get_rng_state().numpy()`), advanced in place.  Returns `raw_vals`, `picked` and `phase_seconds` (wait + score,
        pick, optimise); with picked also `ic_idx`, `ics`, `cand`, `vals`, `info`, `failed`.  Not picked: the scores have no
        spread, the blob is untouched and nothing was optimised - initialize_q_batch's other paths are the caller's."""
        raw = _f64(raw).reshape(-1, self.k)
        n_raw, nr = raw.shape[0], int(num_restarts)
        if not (isinstance(blob, np.ndarray) and blob.dtype == np.uint8 and blob.ndim == 1 and blob.size == TORCH_BLOB_BYTES
                and blob.flags.c_contiguous and blob.flags.writeable):
            raise ValueError(f"blob: a writable contiguous uint8 array of {TORCH_BLOB_BYTES} bytes")
        bounds = _f64(bounds, (2, self.k))
        raw_vals, idx = np.empty(n_raw), np.empty(max(nr, 0), dtype=np.int64)
        ics, cand, vals = np.empty((max(nr, 0), self.k)), np.empty((max(nr, 0), self.k)), np.empty(max(nr, 0))
        ng = (nr + batch_limit - 1) // batch_limit if nr > 0 and batch_limit > 0 else 0
        info = np.zeros((ng, 4), dtype=np.int32)
        failed, picked = C.c_int(0), C.c_int(0)
        clocks = np.zeros(3)
        rc = LIB.pcabo_propose_acqf(self._h, _ptr(raw), n_raw, _ptr(blob), float(eta), nr, int(batch_limit), _ptr(bounds),
                                    int(maxiter), float(best_f), int(bool(maximize)), int(acq), 0 if wake else PROPOSE_NO_WAKE,
                                    _ptr(raw_vals), _ptr(idx), _ptr(ics), _ptr(cand), _ptr(vals), _ptr(info), C.byref(failed),
                                    C.byref(picked), _ptr(clocks))
        self._chk(rc)
        self._keep = None
        out = {"raw_vals": raw_vals, "picked": bool(picked.value), "phase_seconds": clocks}
        if picked.value:
            out.update(ic_idx=idx, ics=ics, cand=cand, vals=vals, info=info, failed=bool(failed.value))
        return out

    # ---- row O --------------------------------------------------------------------------------
    def inverse_map(self, z) -> np.ndarray:
        z = _f64(z).reshape(-1)
        x = np.empty(self.d)
        self._chk(LIB.pcabo_inverse_map(self._h, _ptr(z), _ptr(x)))
        return x

    # ---- introspection / profiling ------------------------------------------------------------
    def gp_state(self):
        n, k = self.n, self.k
        L, R, alpha, ys, nb = np.empty((n, n)), np.empty((n, n)), np.empty(n), np.empty(2), np.empty((2, k))
        self._chk(LIB.pcabo_get_gp_state(self._h, _ptr(L), _ptr(R), _ptr(alpha), _ptr(ys), _ptr(nb)))
        return {"L": np.tril(L), "R": np.tril(R), "alpha": alpha, "y_mean": ys[0], "y_std": ys[1], "norm_bounds": nb}

    def gram(self) -> np.ndarray:
        K = np.empty((self.n, self.n))
        self._chk(LIB.pcabo_get_gram(self._h, _ptr(K)))
        return K

    def set_profiling(self, on: bool) -> None:
        self._chk(LIB.pcabo_set_profiling(self._h, int(bool(on))))

    def reset_profile(self) -> None:
        self._chk(LIB.pcabo_reset_profile(self._h))

    def profile(self) -> dict:
        out = {}
        for i, name in enumerate(PROFILE_GROUPS):
            ms, cnt, by, fl = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_double(0)
            self._chk(LIB.pcabo_get_profile(self._h, i, C.byref(ms), C.byref(cnt), C.byref(by), C.byref(fl)))
            out[name] = {"ms": ms.value, "launches": cnt.value, "bytes": by.value, "flops": fl.value}
        return out

    def profile_calibration(self) -> dict:
        """Milliseconds an event pair reads with nothing in between (subtracted from every profiled pair) and around an
        empty kernel - medians of 64, taken when profiling was switched on."""
        a, b = C.c_double(0), C.c_double(0)
        self._chk(LIB.pcabo_get_profile_calibration(self._h, C.byref(a), C.byref(b)))
        return {"pair_ms": a.value, "empty_kernel_ms": b.value}


class _BorrowedContext(Context):
    """Run b's context inside a Batch: every single-context call works on it; the batch owns and frees it."""

    def __init__(self, handle, max_n, max_d, max_q, device):   # noqa: D401 - no pcabo_ctx_create here
        self._h = C.c_void_p(handle)
        self.max_n, self.max_d, self.max_q, self.device = max_n, max_d, max_q, device
        self.n = self.d = self.k = 0

    def close(self) -> None:
        self._h = C.c_void_p()


class Batch(_Handle):
    """B per-run contexts advancing in lock-step (pcabo_batch_* of include/pcabo.h): one launch sequence for the
    rows A-H of all runs, one scoring launch, shared acquisition launches for the L-BFGS-B rounds of all runs."""
    _last_error, _destroy = LIB.pcabo_batch_last_error, LIB.pcabo_batch_destroy

    def __init__(self, B: int, max_n: int, max_d: int, max_q: int = 512, device: int = 0, workers: int = 0,
                 group_acq: bool = True, device_lbfgsb: int = 0):
        self._create(LIB.pcabo_batch_create, int(device), int(B), int(max_n), int(max_d), int(max_q))
        self.B, self.max_n, self.max_d, self.max_q, self.device = B, max_n, max_d, max_q, device
        self.n = self.d = 0
        self.k = np.zeros(B, dtype=np.int32)
        self.ctx = [_BorrowedContext(LIB.pcabo_batch_ctx(self._h, b), max_n, max_d, max_q, device) for b in range(B)]
        if workers:
            self.set_workers(workers)
        if not group_acq:            # L-BFGS-B rounds through the per-query kernels (a stand-alone context's default)
            self._chk(LIB.pcabo_batch_set_option(self._h, OPT_GROUP_ACQ, 0))
        if device_lbfgsb:            # 1: every restart group's L-BFGS-B inside one launch; 2: its host-stepped twin (tests)
            self._chk(LIB.pcabo_batch_set_option(self._h, OPT_DEVICE_LBFGSB, int(device_lbfgsb)))
        self.device_lbfgsb = int(device_lbfgsb)
        advice = hw_queues_advice(min(B, int(workers) if workers else 8) + 2)      # gang streams + the batch's + the default stream
        if advice:
            import warnings
            warnings.warn(advice, RuntimeWarning, stacklevel=2)

    def set_workers(self, workers: int) -> None:
        """Worker threads of the L-BFGS-B phase (they spin: several batches of one process share the process's cores)."""
        self._chk(LIB.pcabo_batch_set_workers(self._h, int(workers)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            for c in self.ctx:
                c.close()
        super().close()

    @staticmethod
    def _block(a, row):
        """(array, stride between the runs' blocks in doubles) for an input of `row` doubles per run: the blocks as they lie in the
        caller's array - a stride instead of a dense copy - where its layout allows; (None, 0) for None."""
        if a is None:
            return None, 0
        a = np.asarray(a, dtype=np.float64)
        item = a.itemsize
        inner_ok = all(a.strides[i] == item * int(np.prod(a.shape[i + 1:])) for i in range(1, a.ndim))
        if a.dtype == np.float64 and inner_ok and a.strides[0] % item == 0 and a.strides[0] // item >= row:
            return a, a.strides[0] // item
        return np.ascontiguousarray(a, dtype=np.float64), row

    def _packed(self, blocks, row: int) -> np.ndarray:
        """pack_rows into a fresh zeroed buffer with a row for every run."""
        if len(blocks) == self.B:
            return pack_rows(blocks, row)
        return pack_rows(blocks, row, np.zeros((self.B, row)))      # (too few leave rows zero, too many are an IndexError)

    def _input_blocks(self, *inputs):
        """The conditioning calls' (X, noise, y), each given as (array or None, doubles per run), as _block lays them out; the
        library is told the strides between the runs' blocks (0: dense) when they differ from the last call's."""
        arrays, strides = [], []
        for a, row in inputs:
            a, s = self._block(a, row)
            arrays.append(a)
            strides.append(0 if s == row else s)
        strides = tuple(strides)
        if strides != getattr(self, "_in_strides", (0, 0, 0)):
            self._chk(LIB.pcabo_batch_set_input_strides(self._h, *strides))
            self._in_strides = strides
        return arrays

    def wpca_gp_condition_begin(self, X, ranks, noise, y, maximize=False, var_threshold=0.95, n_components=0,
                                lengthscale=0.6931471805599453, gp_noise=0.006737946999085467, kernel=KERNEL_MATERN52):
        """X[B,n,d], ranks[B,n] (int64), noise[B,n,d] or None, y[B,n]: enqueue rows A-H of every run."""
        X = np.asarray(X, dtype=np.float64)
        B, n, d = X.shape
        assert B == self.B
        ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(B, n)
        y = np.asarray(y, dtype=np.float64).reshape(B, n)
        X, nz, y = self._input_blocks((X, n * d), (noise, n * d), (y, n))
        self._chk(LIB.pcabo_batch_wpca_gp_condition_begin(self._h, _ptr(X), _ptr(ranks), _ptr(nz), _ptr(y), n, d,
                                                          int(bool(maximize)), float(var_threshold), int(n_components),
                                                          float(lengthscale), float(gp_noise), int(kernel)))
        self.n, self.d = n, d

    def gp_condition_begin(self, Z, y, norm_bounds=None, lengthscale=0.6931471805599453, gp_noise=0.006737946999085467,
                           kernel=KERNEL_MATERN52):
        """Z[B,n,k], y[B,n]: rows D-H of every run on the given points, no weighted PCA (Vanilla_BO); norm_bounds (2, k) for all
        runs or None.  Finish with gp_wait_eval / gp_eval_begin + gp_eval_end."""
        Z = np.asarray(Z, dtype=np.float64)
        B, n, k = Z.shape
        assert B == self.B
        y = np.asarray(y, dtype=np.float64).reshape(B, n)
        Z, _, y = self._input_blocks((Z, n * k), (None, 0), (y, n))
        nb = None if norm_bounds is None else _f64(norm_bounds, (2, k))
        self._chk(LIB.pcabo_batch_gp_condition_begin(self._h, _ptr(Z), _ptr(y), n, k, _ptr(nb), float(lengthscale), float(gp_noise),
                                                     int(kernel)))
        self.n, self.d = n, k
        self.k = np.full(B, k, dtype=np.int32)
        for c in self.ctx:
            c.n, c.d, c.k = n, k, k

    def wpca_results(self):
        B, n, d = self.B, self.n, self.d
        rc_ = min(n, d)
        dm, pm, comps, evr = np.empty((B, d)), np.empty((B, d)), np.empty((B, d, d)), np.empty((B, d))
        k = np.zeros(B, dtype=np.int32)
        self._chk(LIB.pcabo_batch_wpca_results(self._h, _ptr(dm), _ptr(pm), _ptr(comps), _ptr(evr), _ptr(k)))
        self.k = k
        for b, c in enumerate(self.ctx):
            c.n, c.d, c.k = n, d, int(k[b])
        return [{"data_mean": dm[b], "pca_mean": pm[b], "components": comps[b].reshape(-1)[: rc_ * d].reshape(rc_, d),
                 "evr": evr[b, :rc_], "k": int(k[b]), "Z": None} for b in range(B)]

    def acq_bounds(self):
        buf = self.acq_bounds_packed = np.zeros((self.B, 2 * self.max_d))     # (kept: sobol_draw_rows reads the boxes from it)
        self._chk(LIB.pcabo_batch_acq_bounds(self._h, _ptr(buf)))
        return [buf[b, : 2 * int(self.k[b])].reshape(2, int(self.k[b])).copy() for b in range(self.B)]

    def gp_wait_eval(self, Xq_list, best_f, maximize=False, acq=ACQ_LOG_EI):
        """Xq_list[b]: q x k_b points of run b; best_f[B]: every run's scalar (ACQ_UCB: its kappa = sqrt(beta), as in
        Context.acq_eval - the same holds for every `best_f` of this class).  Returns (values[B, q], status[B])."""
        q = Xq_list[0].shape[0]
        buf = self._packed(Xq_list, q * self.max_d)
        bf = _f64(best_f, (self.B,))
        val = np.empty((self.B, q))
        status = np.zeros(self.B, dtype=np.int32)
        self._chk(LIB.pcabo_batch_gp_condition_end_eval(self._h, _ptr(buf), q, _ptr(bf), int(bool(maximize)), int(acq),
                                                        _ptr(val), _ptr(status)))
        return val, status

    def gp_posterior(self, Xq_list, observation_noise=False, covariance=False):
        """Context.gp_posterior for every run in one launch sequence (Xq_list[b]: q x k_b, the same q for all runs; the batch's
        conditioning has been waited for).  One dict per run, None for a run that was skipped (parked, or without a GP)."""
        q = Xq_list[0].shape[0]
        buf = self._packed(Xq_list, q * self.max_d)
        mean, var = np.zeros((self.B, q)), np.zeros((self.B, q))
        cov = np.zeros((self.B, q, q)) if covariance else None
        status = np.zeros(self.B, dtype=np.int32)
        self._chk(LIB.pcabo_batch_gp_posterior(self._h, _ptr(buf), q, POST_OBS_NOISE if observation_noise else 0, _ptr(mean),
                                               _ptr(var), _ptr(cov), _ptr(status)))
        def one(b):
            out = {"mean": mean[b].copy(), "variance": var[b].copy()}
            if covariance:
                out["covariance"] = cov[b].copy()
            return out
        return per_run(status, one)

    def gp_loo(self):
        """Context.gp_loo for every run in one launch (the batch's conditioning has been waited for).  One dict per run, None for
        a run that was skipped (parked, or without a GP)."""
        n = self.n
        mean, var, z, lpd = (np.zeros((self.B, n)) for _ in range(4))
        total = np.zeros(self.B)
        status = np.zeros(self.B, dtype=np.int32)
        self._chk(LIB.pcabo_batch_gp_loo(self._h, _ptr(mean), _ptr(var), _ptr(z), _ptr(lpd), _ptr(total), _ptr(status)))
        return per_run(status, lambda b: {"mean": mean[b].copy(), "variance": var[b].copy(), "z": z[b].copy(),
                                          "lpd": lpd[b].copy(), "lpd_sum": float(total[b])})

    def gp_posterior_samples(self, Xq_list, n_samples=None, base_samples=None, seed=None, observation_noise=False, centred=False):
        """Context.gp_posterior_samples for every run in one launch sequence (Xq_list[b]: q x k_b, the same q for all runs).
        base_samples: (S, q) for all runs or (B, S, q); with n_samples every run gets the same seeded base.  One dict per run, None
        for a run that was skipped (parked, without a GP, or with a covariance no rung could factor); `status` keeps the codes."""
        q = Xq_list[0].shape[0]
        if base_samples is not None and np.ndim(base_samples) == 3:
            if seed is not None or n_samples is not None:
                raise ValueError("give exactly one of n_samples and base_samples")
            base = np.ascontiguousarray(base_samples, dtype=np.float64)
            if base.shape[0] != self.B or base.shape[2] != q or base.shape[1] < 1:
                raise ValueError(f"base_samples must be B x S x q = {self.B} x S x {q}, got {base.shape}")
        else:
            one = sample_base(q, n_samples, base_samples, seed)
            base = np.ascontiguousarray(np.broadcast_to(one, (self.B,) + one.shape))
        S = base.shape[1]
        buf = self._packed(Xq_list, q * self.max_d)
        samples, mean, jitter = np.zeros((self.B, S, q)), np.zeros((self.B, q)), np.zeros(self.B)
        status = self.sample_status = np.zeros(self.B, dtype=np.int32)
        flags = (POST_OBS_NOISE if observation_noise else 0) | (POST_CENTRED if centred else 0)
        self._chk(LIB.pcabo_batch_gp_posterior_sample(self._h, _ptr(buf), q, flags, _ptr(base), S, _ptr(samples), _ptr(mean),
                                                      _ptr(jitter), _ptr(status)))
        return per_run(status, lambda b: {"samples": samples[b].copy(), "mean": mean[b].copy(), "jitter": float(jitter[b])})

    # ---- appending points to every run's GP and taking them back (pcabo_batch_gp_extend / pcabo_batch_gp_truncate) -------
    def _counts(self):
        nb, n = C.c_int(0), C.c_int(0)
        self._chk(LIB.pcabo_batch_gp_extended(self._h, C.byref(nb), C.byref(n)))
        return int(nb.value), int(n.value)

    def _follow_n(self, held=None) -> int:
        """The batch's n as the library holds it, for this object; the runs' borrowed contexts get the number of points they hold
        (held[b]; None: the batch's n for all) - a run set aside by gp_extend holds fewer, and its gp_state() reads those."""
        self.n = self._counts()[1]
        for b, c in enumerate(self.ctx):
            c.n = self.n if held is None else int(held[b])
        return self.n

    def _chk_fit(self, rc: int) -> None:
        """_chk for a fit or likelihood evaluation: they forget points appended by gp_extend and bring every run back in step, so n
        follows the library; a refused call changed nothing, and then only the batch's own n is read again."""
        try:
            self._chk(rc)
        except PcaboError:
            self.n = self._counts()[1]
            raise
        self._follow_n()

    def gp_extend(self, Zp_list, y=None):
        """Context.gp_extend for every run in one launch sequence per point: Zp_list[b] is p x k_b (None for a run the caller knows
        to be skipped), y is (B, p), or None for believer mode.  Returns (n, status[B]): 0 for a run that took the points, -1 for
        a run that took no part (parked, without a GP, set aside), -2 for a run whose pivot failed - it alone is taken back and set
        aside until gp_truncate reaches the n of entry (include/pcabo.h)."""
        if len(Zp_list) != self.B:
            raise ValueError(f"Zp_list must have one entry per run ({self.B})")
        Zp = [None if z is None else np.asarray(z, dtype=np.float64).reshape(-1, int(self.k[b])) for b, z in enumerate(Zp_list)]
        shapes = {z.shape[0] for z in Zp if z is not None}
        if len(shapes) > 1:
            raise ValueError("every run takes the same number of points")
        p = shapes.pop() if shapes else (0 if y is None else np.asarray(y).reshape(self.B, -1).shape[1])
        buf = self._packed(Zp, max(p, 1) * self.max_d)
        yv = None if y is None else _f64(y, (self.B, p))
        status = np.zeros(self.B, dtype=np.int32)
        self._chk(LIB.pcabo_batch_gp_extend(self._h, _ptr(buf), _ptr(yv), p, EXTEND_BELIEVER if y is None else 0,
                                            _ptr(status)))
        new_n = self._counts()[1]
        return self._follow_n([new_n if status[b] == 0 else c.n for b, c in enumerate(self.ctx)]), status

    def gp_truncate(self, n0=None) -> int:
        """Take back the appended points of every run from n0 on (None: all of them, back to n_base).  Returns the new n."""
        n0 = self.n_base if n0 is None else int(n0)
        self._chk(LIB.pcabo_batch_gp_truncate(self._h, n0, None))
        return self._follow_n([min(c.n, n0) for c in self.ctx])

    @property
    def n_base(self) -> int:
        """The n of the batch's last conditioning or fit: gp_extend appends behind it."""
        return self._counts()[0]

    # ---- opt-in GP hyperparameter fit of all runs in lock-step (pcabo_batch_gp_mll / pcabo_batch_gp_fit) -----------------
    # Both work on the inputs of the last wpca_gp_condition_begin / gp_condition_begin and leave every run conditioned at its
    # own theta; gp_wait_eval / gp_eval_begin + gp_eval_end and optimize_acqf then use the runs' own models.
    def _fit_call(self, fn, key, th, ks=None):
        """One of the four calls on the packed thetas `th`, and its results: per run fit_result with `grad` (key "grad") or with
        the fit's counters (key "info"), plus `status` 0; only `status` for a run the call skipped.  ks: the runs' k in the
        per-input form (rows of 2 + max k, whose width the library is told), None in the shared form (rows of 3)."""
        ard = ks is not None
        loss, status = np.zeros(self.B), np.zeros(self.B, dtype=np.int32)
        extra = np.zeros_like(th) if key == "grad" else np.zeros((self.B, 4), dtype=np.int32)
        width = (th.shape[1],) if ard else ()
        self._chk_fit(fn(self._h, _ptr(th), *width, _ptr(loss), _ptr(extra), _ptr(status)))
        if ard or key == "info":                        # (the shared form's likelihood steps no rounds)
            self.fit_rounds = int(LIB.pcabo_batch_gp_fit_rounds(self._h))

        def one(b):
            w = 2 + ks[b] if ard else 3
            return {**fit_result(th[b, :w], loss[b], ard, **{key: extra[b, :w].copy() if key == "grad" else extra[b]}), "status": 0}
        return per_run(status, one, status_only=True)

    def gp_mll(self, thetas):
        """thetas (B, 3) = (noise, mean constant, raw lengthscale) per run.  One dict per run as Context.gp_mll returns it, plus
        `status` (0; a parked run or one that could not be factored: only `status`)."""
        return self._fit_call(LIB.pcabo_batch_gp_mll, "grad", _f64(thetas, (self.B, 3)))

    def gp_fit(self, theta0=None):
        """Fit every run's (noise, mean constant, raw lengthscale) from theta0 ((3,) for all runs, (B, 3), or None: the model's
        initial values), all runs stepped side by side, one launch sequence per round; bit for bit the fits Context.gp_fit
        finds for the runs one by one.  One dict per run as Context.gp_fit returns it, plus `status` (a parked run, or one whose
        start could not be factored: only `status`).  `fit_rounds`: the launch sequences the call took."""
        th0 = np.asarray(FIT_THETA0 if theta0 is None else theta0, dtype=np.float64)
        th = np.ascontiguousarray(np.broadcast_to(th0, (self.B, 3)), dtype=np.float64).copy()
        return self._fit_call(LIB.pcabo_batch_gp_fit, "info", th)

    # ---- the same with one lengthscale per input (pcabo_batch_gp_mll_ard / pcabo_batch_gp_fit_ard) ------------------------
    def _ard_rows(self, thetas):
        """(B, 2 + max k) rows for the library from one theta per run (None: the model's initial values), and the runs' k."""
        ks = [int(k) for k in self.k]
        if min(ks) < 1:
            raise ValueError("the runs' reduced dimensions are not known yet: collect wpca_results() first")
        rows = np.zeros((self.B, 2 + max(ks)))
        for b, k in enumerate(ks):
            rows[b, : 2 + k] = Context._theta(None if thetas is None else thetas[b], k, True)
        return rows, ks

    def gp_mll_ard(self, thetas):
        """thetas[b] (2 + k_b,) = (noise, mean constant, rho_1 .. rho_{k_b}) of run b.  One dict per run as Context.gp_mll_ard
        returns it (`theta` and `grad` of length 2 + k_b), plus `status` (0; a parked run or one that could not be factored:
        only `status`)."""
        return self._fit_call(LIB.pcabo_batch_gp_mll_ard, "grad", *self._ard_rows(thetas))

    def gp_fit_ard(self, theta0=None):
        """Batch.gp_fit with one lengthscale per input: theta0[b] (2 + k_b,) per run, or None: the model's initial values (every
        rho_c = 0).  Bit for bit the fits Context.gp_fit_ard finds for the runs one by one; one dict per run as it returns it,
        plus `status`.  `fit_rounds`: the launch sequences the call took."""
        return self._fit_call(LIB.pcabo_batch_gp_fit_ard, "info", *self._ard_rows(theta0))

    # ---- the two waiting calls in halves (one thread advancing several batches: pcabo.batchrun.run_interleaved) -------------
    def busy(self) -> bool:
        rc = LIB.pcabo_batch_busy(self._h)
        if rc < 0:
            raise PcaboError(rc, self._err())
        return rc == 1

    def raw_row_buffer(self, q: int) -> np.ndarray:
        """The (B, q * max_d) buffer gp_eval_begin and acq_score_begin pack the runs' points into: a caller that writes run b's
        q x k_b points into `buf[b, :q*k_b].reshape(q, k_b)` itself (and passes those views) saves the copy.  Kept from call to
        call and never cleared: only the first q * k_b entries of a row are read, no need to clear 5 MB per call."""
        buf = getattr(self, "_raw_buf", None)
        if buf is None or buf.shape != (self.B, q * self.max_d):
            buf = self._raw_buf = np.zeros((self.B, q * self.max_d))
        return buf

    def gp_eval_begin(self, Xq_list, best_f, maximize=False, acq=ACQ_LOG_EI):
        q = Xq_list[0].shape[0]
        buf = pack_rows(Xq_list, q * self.max_d, self.raw_row_buffer(q))
        bf = _f64(best_f, (self.B,))
        self._chk(LIB.pcabo_batch_gp_condition_end_eval_begin(self._h, _ptr(buf), q, _ptr(bf), int(bool(maximize)), int(acq)))
        return (buf, q, bf, int(bool(maximize)), int(acq))

    def gp_eval_end(self, token):
        buf, q, bf, mx, acq = token
        val = np.empty((self.B, q))
        status = np.zeros(self.B, dtype=np.int32)
        self._chk(LIB.pcabo_batch_gp_condition_end_eval_end(self._h, _ptr(buf), q, _ptr(bf), mx, acq, _ptr(val), _ptr(status)))
        return val, status

    # ---- values on the model as it stands (pcabo_batch_acq_score: the later proposals of an iteration) ---------------------
    def acq_score_begin(self, Xq_list, best_f, maximize=False, acq=ACQ_LOG_EI):
        """Enqueue the scoring of Xq_list[b] (q x k_b, the same q for all runs) on every run's current model - extended or not,
        fitted or not; the batch's conditioning has been waited for.  Returns the token acq_score_end takes."""
        q = Xq_list[0].shape[0]
        buf = pack_rows(Xq_list, q * self.max_d, self.raw_row_buffer(q))
        bf = _f64(best_f, (self.B,))
        self._chk(LIB.pcabo_batch_acq_score_begin(self._h, _ptr(buf), q, _ptr(bf), int(bool(maximize)), int(acq)))
        return q

    def acq_score_end(self, token):
        """(values[B, q], status[B]): status -1 for a run that was skipped (parked, set aside, without a GP), its row zeros."""
        q = token
        val, status = np.zeros((self.B, q)), np.zeros(self.B, dtype=np.int32)
        self._chk(LIB.pcabo_batch_acq_score_end(self._h, q, _ptr(val), _ptr(status)))
        return val, status

    def acq_score(self, Xq_list, best_f, maximize=False, acq=ACQ_LOG_EI):
        return self.acq_score_end(self.acq_score_begin(Xq_list, best_f, maximize, acq))

    def _pack_ics(self, ics_list, bounds_list):
        nr = ics_list[0].shape[0]
        return nr, self._packed(ics_list[: self.B], nr * self.max_d), self._packed(bounds_list[: self.B], 2 * self.max_d)

    def optimize_begin(self, ics_list, bounds_list, best_f, maximize=False, acq=ACQ_LOG_EI, batch_limit=5, maxiter=200):
        """Enqueue the device-resident optimisation; returns a token for optimize_end, or None when the call does not qualify
        (the caller then uses optimize_acqf)."""
        nr, ics, bnd = self._pack_ics(ics_list, bounds_list)
        bf = _f64(best_f, (self.B,))
        rc = LIB.pcabo_batch_optimize_acqf_begin(self._h, _ptr(ics), nr, int(batch_limit), _ptr(bnd), int(maxiter), _ptr(bf),
                                                 int(bool(maximize)), int(acq))
        if rc == 1:
            return None
        self._chk(rc)
        return (nr, int(batch_limit))

    def _optimise_outputs(self, nr, batch_limit):
        """The buffers an optimise call fills (candidates, values, counters per restart group, retry flags, status per run)."""
        B, ng = self.B, (nr + batch_limit - 1) // batch_limit
        return (np.zeros((B, nr * self.max_d)), np.zeros((B, nr)), np.zeros((B, ng, 4), dtype=np.int32),
                np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32))

    def _unpack_optimised(self, nr, cand, vals, info, failed):
        """Per run (cand nr x k_b, vals, info, failed) out of the packed rows."""
        out = []
        for b in range(self.B):
            k = int(self.k[b])
            out.append((cand[b, : nr * k].reshape(nr, k).copy(), vals[b].copy(), info[b].copy(), bool(failed[b])))
        return out

    def optimize_end(self, token):
        nr, batch_limit = token
        cand, vals, info, failed, status = self._optimise_outputs(nr, batch_limit)
        self._chk(LIB.pcabo_batch_optimize_acqf_end(self._h, nr, batch_limit, _ptr(cand), _ptr(vals), _ptr(info), _ptr(failed), _ptr(status)))
        return self._unpack_optimised(nr, cand, vals, info, failed), status

    def optimize_acqf(self, ics_list, bounds_list, best_f, maximize=False, acq=ACQ_LOG_EI, batch_limit=5, maxiter=200):
        """ics_list[b]: num_restarts x k_b; bounds_list[b]: 2 x k_b.  Returns per run (cand, vals, info, failed) + status."""
        nr, ics, bnd = self._pack_ics(ics_list, bounds_list)
        bf = _f64(best_f, (self.B,))
        cand, vals, info, failed, status = self._optimise_outputs(nr, batch_limit)
        self._chk(LIB.pcabo_batch_optimize_acqf(self._h, _ptr(ics), nr, int(batch_limit), _ptr(bnd), int(maxiter), _ptr(bf),
                                                int(bool(maximize)), int(acq), _ptr(cand), _ptr(vals), _ptr(info),
                                                _ptr(failed), _ptr(status)))
        return self._unpack_optimised(nr, cand, vals, info, failed), status

    def device_acq_eval(self, xq_list, best_f, maximize=False, acq=ACQ_LOG_EI):
        """Value and gradient at xq_list[b] (q x k_b, q <= 32) through the evaluation of the device-resident optimiser."""
        B, MD = self.B, self.max_d
        q = xq_list[0].shape[0]
        xq = self._packed(xq_list[:B], q * MD)
        bf = _f64(best_f, (B,))
        val, grad = np.zeros((B, q)), np.zeros((B, q * MD))
        self._chk(LIB.pcabo_batch_device_acq_eval(self._h, _ptr(xq), int(q), _ptr(bf), int(bool(maximize)), int(acq), _ptr(val), _ptr(grad)))
        return [val[b].copy() for b in range(B)], [grad[b, : q * int(self.k[b])].reshape(q, int(self.k[b])).copy() for b in range(B)]

    def twin_branches(self):
        """After a twin call (device_lbfgsb = 2) of optimize_acqf: per run a list with one dict per restart group, the host
        optimiser's branch counters (LBFGSB_BRANCHES)."""
        nb = len(LBFGSB_BRANCHES)
        buf = np.zeros(self.B * 32 * nb, dtype=np.uint32)
        ng = LIB.pcabo_debug_batch_lbfgsb_branches(self._h, _ptr(buf), int(buf.size))
        if ng <= 0:
            raise PcaboError(-1, "twin_branches: the last optimise call of this batch was no twin call")
        arr = buf[: self.B * ng * nb].reshape(self.B, ng, nb)
        return [[dict(zip(LBFGSB_BRANCHES, (int(v) for v in arr[b, gi]))) for gi in range(ng)] for b in range(self.B)]

    def device_group_out(self):
        """After a device-mode call (device_lbfgsb = 1) of optimize_acqf / optimize_end: per run a list with one dict per restart
        group of what the kernel wrote for it (DEVICE_GROUP_FIELDS)."""
        buf = np.zeros(self.B * 32 * 8)
        ng = LIB.pcabo_debug_batch_lbfgsb_device_out(self._h, _ptr(buf), int(buf.size))
        if ng <= 0:
            raise PcaboError(-1, "device_group_out: the last optimise call of this batch did not run on the device")
        arr = buf[: self.B * ng * 8].reshape(self.B, ng, 8)
        return [[dict(zip(DEVICE_GROUP_FIELDS, (int(v) for v in arr[b, gi]))) for gi in range(ng)] for b in range(self.B)]

    def set_profiling(self, on: bool) -> None:
        self._chk(LIB.pcabo_batch_set_profiling(self._h, int(bool(on))))

    def set_active(self, active) -> None:
        """active[b] = False parks run b: it stays in the lock-step launches but is skipped by optimize_acqf."""
        a = np.ascontiguousarray(active, dtype=np.int32).reshape(self.B)
        self._chk(LIB.pcabo_batch_set_active(self._h, _ptr(a)))

    def condition_profile(self) -> dict:
        """Device milliseconds of the last conditioning's phases (after it has been waited for)."""
        ms = np.zeros(4)
        self._chk(LIB.pcabo_batch_get_profile(self._h, _ptr(ms)))
        return dict(zip(("wpca", "gram", "cholesky", "root_inverse_alpha"), ms.tolist()))

    def inverse_map(self, z_list):
        z = self._packed(z_list, self.max_d)
        x = np.empty((self.B, self.d))
        self._chk(LIB.pcabo_batch_inverse_map(self._h, _ptr(z), _ptr(x)))
        return x

    def inverse_map_begin(self, z_list) -> None:
        z = self._packed(z_list, self.max_d)
        self._chk(LIB.pcabo_batch_inverse_map_begin(self._h, _ptr(z)))

    def inverse_map_end(self):
        x = np.empty((self.B, self.d))
        self._chk(LIB.pcabo_batch_inverse_map_end(self._h, _ptr(x)))
        return x


def sobol_scramble(state: np.ndarray, ltm: np.ndarray) -> None:
    """In-place scramble of a (k, 30) int64 Sobol state with (k, 30, 30) int64 lower-triangular bit matrices."""
    assert state.dtype == np.int64 and ltm.dtype == np.int64 and state.flags.c_contiguous and ltm.flags.c_contiguous
    rc = LIB.pcabo_sobol_scramble(_ptr(state), _ptr(ltm), int(state.shape[0]))
    if rc != 0:
        raise PcaboError(rc, "pcabo_sobol_scramble: bad argument")


def sobol_draw(state: np.ndarray, shift: np.ndarray, n: int, lo=None, rng=None, out=None) -> np.ndarray:
    """n points of a fresh scrambled engine ((k, 30) int64 state after `sobol_scramble`, (k,) int64 shift), optionally mapped
    into the box lo + rng * u - bit-identical to torch's SobolEngine.draw + botorch's scaling (pcabo_sobol_draw)."""
    assert state.dtype == np.int64 and shift.dtype == np.int64 and state.flags.c_contiguous and shift.flags.c_contiguous
    k = int(state.shape[0])
    if out is None:
        out = np.empty((int(n), k))
    else:
        assert out.shape == (int(n), k) and out.dtype == np.float64 and out.flags.c_contiguous
    if lo is not None:
        lo, rng = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(rng, dtype=np.float64)
    rc = LIB.pcabo_sobol_draw(_ptr(state), _ptr(shift), k, int(n), _ptr(lo), _ptr(rng), _ptr(out))
    if rc != 0:
        raise PcaboError(rc, "pcabo_sobol_draw: bad argument")
    return out


def sobol_draw_rows(engines, n: int, boxes: np.ndarray, outbuf: np.ndarray):
    """`sobol_draw` for the runs of a batch in one native call (pcabo_sobol_draw_rows): engines[b] (objects with .k, .state, .shift;
    None = skip) draws n points into `outbuf[b, :n*k_b]`, mapped into the box packed in `boxes[b]` as [lo(k_b), hi(k_b)]
    (Batch.acq_bounds_packed).  Returns the list of (n, k_b) views into `outbuf` (None for skipped runs)."""
    B = len(engines)
    assert boxes.dtype == np.float64 and boxes.flags.c_contiguous and boxes.shape[0] == B
    assert outbuf.dtype == np.float64 and outbuf.flags.c_contiguous and outbuf.shape[0] == B
    ks = np.zeros(B, dtype=np.int32)
    st, sh, ou = (C.c_void_p * B)(), (C.c_void_p * B)(), (C.c_void_p * B)()
    base, stride = outbuf.ctypes.data, outbuf.strides[0]
    views = [None] * B
    for b, e in enumerate(engines):
        if e is None:
            continue
        k = ks[b] = e.k
        assert 2 * k <= boxes.shape[1] and n * k <= outbuf.shape[1] and e.state.dtype == np.int64 and e.shift.dtype == np.int64
        st[b], sh[b], ou[b] = e.state.ctypes.data, e.shift.ctypes.data, base + b * stride
        views[b] = outbuf[b, : n * k].reshape(n, k)
    rc = LIB.pcabo_sobol_draw_rows(st, sh, _ptr(ks), B, int(n), _ptr(boxes), boxes.strides[0] // 8, ou)
    if rc != 0:
        raise PcaboError(rc, "pcabo_sobol_draw_rows: bad argument")
    return views


def comm_unique_id() -> bytes:
    """128 bytes (ncclUniqueId) from rank 0 for `Comm`; the caller distributes them to the other ranks."""
    buf = C.create_string_buffer(128)
    rc = LIB.pcabo_comm_unique_id(buf)
    if rc != 0:
        raise PcaboError(rc, "librccl.so could not be opened or ncclGetUniqueId failed")
    return buf.raw


class Comm(_Handle):
    """RCCL communicator for the final gather of best-so-far values (pcabo_comm_* / pcabo_gather_best of include/pcabo.h)."""
    _last_error, _destroy = LIB.pcabo_comm_last_error, LIB.pcabo_comm_destroy
    _NOT_CREATED = "librccl.so could not be opened"

    def __init__(self, unique_id: bytes, world: int, rank: int, device: int = 0):
        self._create(LIB.pcabo_comm_create, C.c_char_p(unique_id), int(world), int(rank), int(device))
        self.world, self.rank = int(world), int(rank)

    def gather_best(self, local) -> np.ndarray:
        local = _f64(local).reshape(-1)
        out = np.empty((self.world, local.shape[0]))
        self._chk(LIB.pcabo_gather_best(self._h, _ptr(local), int(local.shape[0]), _ptr(out)))
        return out


def lbfgsb_set_vector_kernels(enabled: bool) -> bool:
    """Host L-BFGS-B: AVX2 (default) or scalar O(m n) loops - same iterates; returns the previous setting (tests)."""
    return bool(LIB.pcabo_lbfgsb_set_vector_kernels(int(bool(enabled))))


def lbfgsb_set_sum_order(order: int) -> int:
    """0: the published summation order (scipy's iterates), 1: the device optimiser's 64-lane tree order.  Returns the previous one."""
    return int(LIB.pcabo_lbfgsb_set_sum_order(int(order)))


def lbfgsb_minimize(fun, x0, bounds, m=10, factr=1e7, pgtol=1e-5, maxiter=15000, maxfun=15000, maxls=20):
    """Host-only entry: this library's L-BFGS-B on a Python objective `fun(x) -> (f, g)` (for tests)."""
    x = _f64(x0).reshape(-1).copy()
    nvar = x.shape[0]
    lo = _f64([b[0] if b[0] is not None else -np.inf for b in bounds])
    hi = _f64([b[1] if b[1] is not None else np.inf for b in bounds])

    def cb(xp, gp, _user):
        xv = np.ctypeslib.as_array(xp, shape=(nvar,))
        f, g = fun(xv.copy())
        np.ctypeslib.as_array(gp, shape=(nvar,))[:] = g
        return float(f)

    cfun = FG_CALLBACK(cb)
    f_out, nit, nfev, task = C.c_double(0), C.c_int(0), C.c_int(0), C.c_int(0)
    warn = LIB.pcabo_lbfgsb_minimize(nvar, _ptr(x), _ptr(lo), _ptr(hi), cfun, None, int(m), float(factr), float(pgtol),
                                     int(maxiter), int(maxfun), int(maxls), C.byref(f_out), C.byref(nit),
                                     C.byref(nfev), C.byref(task))
    br = np.zeros(len(LBFGSB_BRANCHES), dtype=np.uint32)
    LIB.pcabo_debug_lbfgsb_branches(_ptr(br), int(br.size))
    return {"x": x, "fun": f_out.value, "nit": nit.value, "nfev": nfev.value, "warnflag": warn, "task": task.value,
            "branches": dict(zip(LBFGSB_BRANCHES, (int(v) for v in br)))}
