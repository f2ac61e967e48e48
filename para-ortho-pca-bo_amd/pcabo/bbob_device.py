"""Device-side evaluation of the BBOB f15-f24 objectives for runs that advance in lock-step.

The seeded tables of a problem (x_opt, rotations, conditioning, Gallagher peaks) come from `pcabo.bbob` - the legacy
generators are sequential integer recurrences and run once per run on the host - and are uploaded once; the B candidates
of a lock-step iteration are then evaluated in ONE launch (`pcabo_bbob_eval`, csrc/kernels_bbob.hip), which also applies
PCA_BO's out-of-box rule (reference PCA_BO.py:248-263).  Values are those of the definitions to within the worst-case
float64 error bound of tests/bbob_reference.py (1 unit; measured on an MI355X over d = 2 ... 128, worst per function:
f15 0.21, f16 0.66, f17 0.87, f18 0.81, f19 0.27, f20 0.61, f21 0.81, f22 0.74, f23 0.51, f24 0.21; `BBOBProblem.raw`
0.13 ... 0.38 - EXPERIMENTS.md section 29), in another summation order than the host's, so not bit-equal to it; the host
evaluation stays the default of `pcabo.batchrun` so that a batched run is bit-identical to the same run alone.  Per-run table layout (doubles): [x_opt(d) | R(d*d) | M(d*d) | aux(101*(2d+1) + 4d + 8)]."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native
from .bbob import BBOBProblem

_PEAKS = 101


def _table(p: BBOBProblem, stride: int) -> np.ndarray:
    st, d, fid = p._state, int(p.meta_data.n_variables), int(p.meta_data.problem_id)
    t = np.zeros(stride)
    xo, r, m, aux = 0, d, d + d * d, d + 2 * d * d
    put = lambda off, a: t.__setitem__(slice(off, off + np.asarray(a).size), np.asarray(a, dtype=np.float64).ravel())
    if fid in (15, 16, 17, 18, 23):
        put(xo, st.xopt); put(r, st.rot_r); put(m, st.m)
    elif fid == 19:
        put(m, st.m)
    elif fid == 20:
        put(aux, st.sign); put(aux + d, st.offset); put(aux + 2 * d, st.cond)
    elif fid in (21, 22):
        put(r, st.rot)
        P = st.peaks
        put(aux, st.heights); put(aux + _PEAKS, st.scales); put(aux + _PEAKS + _PEAKS * d, st.centres)
        assert P <= _PEAKS
    elif fid == 24:
        put(xo, st.xopt); put(r, st.rot_r); put(m, st.rot_q); put(aux, st.cond)
    else:
        raise NotImplementedError(fid)
    return t


class DeviceObjectives(_native._Handle):
    """`problems`: B `BBOBProblem`s of one dimension.  `evaluate(X[B, d])` -> (f[B] incl. f_opt, or the penalty for a
    candidate outside [lb, ub]^d; raw[B] without f_opt, the penalty likewise; oob[B] bool).  `lb`, `ub` and `penalty` are
    read at every call."""
    _destroy = _native.LIB.pcabo_bbob_destroy           # (no last-error call: a failed creation has one text)
    _NOT_CREATED = "pcabo_bbob_create failed (no usable HIP device?)"

    def __init__(self, problems, device: int = 0, penalty: float = 1000.0):
        self.problems = list(problems)
        self.B = len(self.problems)
        self.d = int(self.problems[0].meta_data.n_variables)
        assert all(int(p.meta_data.n_variables) == self.d for p in self.problems)
        stride = _native.LIB.pcabo_bbob_table_doubles(self.d)
        if stride < 0:
            raise _native.PcaboError(stride, "dimension not supported by the device objectives")
        tables = np.stack([_table(p, stride) for p in self.problems])
        fid = np.array([int(p.meta_data.problem_id) for p in self.problems], dtype=np.int32)
        self.f_opt = np.array([p.f_opt for p in self.problems])
        self.lb, self.ub = float(self.problems[0].bounds.lb[0]), float(self.problems[0].bounds.ub[0])
        self.penalty = float(penalty)
        self._create(_native.LIB.pcabo_bbob_create, int(device), self.B, self.d, fid.ctypes.data_as(C.c_void_p),
                     tables.ctypes.data_as(C.c_void_p))

    def evaluate(self, X: np.ndarray):
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(self.B, self.d)
        raw, oob = np.empty(self.B), np.zeros(self.B, dtype=np.int32)
        rc = _native.LIB.pcabo_bbob_eval(self._h, X.ctypes.data_as(C.c_void_p), self.lb, self.ub, self.penalty,
                                         raw.ctypes.data_as(C.c_void_p), oob.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise _native.PcaboError(rc, "pcabo_bbob_eval failed")
        f = np.where(oob != 0, self.penalty, raw + self.f_opt)
        return f, raw, oob.astype(bool)

    def eval_many(self, X: np.ndarray):
        """evaluate() for m candidates per run in one launch: X[B, m, d] -> (f[B, m], raw[B, m], oob[B, m]); candidate j of run b
        as evaluate() gives it alone (`pcabo_bbob_eval_many`)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 3 or X.shape[0] != self.B or X.shape[2] != self.d:
            raise ValueError(f"eval_many takes X[B, m, d] = [{self.B}, m, {self.d}], got {X.shape}")
        m = X.shape[1]
        raw, oob = np.empty((self.B, m)), np.zeros((self.B, m), dtype=np.int32)
        rc = _native.LIB.pcabo_bbob_eval_many(self._h, X.ctypes.data_as(C.c_void_p), m, self.lb, self.ub, self.penalty,
                                              raw.ctypes.data_as(C.c_void_p), oob.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise _native.PcaboError(rc, "pcabo_bbob_eval_many failed")
        f = np.where(oob != 0, self.penalty, raw + self.f_opt[:, None])
        return f, raw, oob.astype(bool)
