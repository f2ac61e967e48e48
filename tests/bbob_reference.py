"""Extended-precision reference of the BBOB objectives f15-f24 and the error unit their evaluations are judged in.

No tests here: `test_bbob_reference_cpu.py` proves the reference, its unit and the grid's sensitivity on the host
restatement (`pcabo.bbob`), `test_gpu_bbob_edges.py` judges the HIP kernel `k_bbob_eval` (csrc/kernels_bbob.hip) by them.

The ten functions are restated from the published definitions (Hansen, Finck, Ros, Auger 2009, "Real-parameter black-box
optimization benchmarking 2009: noiseless functions definitions", in the form the legacy code evaluates them, as quoted in
the docstrings of `pcabo/bbob.py`).  Nothing of `pcabo.bbob`'s arithmetic is called: neither its `*_raw` functions nor
`_t_osz` / `_t_asy`.  The inputs are the operands the kernel gets - a problem's seeded float64 tables from
`BBOBProblem._state` (data, the same for every implementation) and the point x.

Arithmetic: `np.longdouble` (64-bit mantissa on x86); the same formulas run on `mpmath.mpf` objects with
`evaluate(..., backend="mp")`, which is how the CPU test guards against long-double libm surprises.

Every quantity is a pair `Q(v, u)`: the value and a first-order bound on the error of ANY float64 evaluation of the same
formula.  E = 2**-53 (one correctly rounded operation has relative error <= E).  None of the rules comes from a run of the
code under test:
  a + b             u_a + u_b + min(E |v|, |a| + u_a, |b| + u_b)      (the rounding of a sum is at most its smaller operand)
  a * b, a / b      first-order terms + u_a u_b + E |v|; no E |v| for a product with an exact power of two
  constants         a decimal constant (0.1, 0.49, 418.98..., 2 pi) carries its own float64 rounding |c - fl(c)|
  g(v), g smooth    |g'(v)| u + C E |g(v)|, with C = C_LIBM = 4 for log / exp / sin / cos / pow, C = 1 for sqrt.
                    4 E is 2 ulp: glibc documents <= 1 ulp for these five in double precision on x86-64, and the device
                    library evaluates pow on a double-double logarithm and reduces sin / cos arguments exactly
                    (Payne-Hanek), so their own errors are of the same size; the rounding of an amplified inner argument
                    (t = log|x| / 0.1 feeding sin in T_osz, 2 pi 3^k (z + 1/2) in Weierstrass, the exponent of T_asy) is
                    carried by the argument's own u, which the |g'| term amplifies.  The second-order term u^2 is added
                    for sin / cos / exp.  exp(0) = 1, cos(0) = 1 and pow(1, p) = 1 are exact (C Annex F), so an exact
                    argument there gives an exact result.
  A v, d terms      |A| u + (d + 1) E |A| |v|                          (any summation order, FMA contraction)
  n-term sum        sum u + n E sum |term|
  |t - round(t)|    1-Lipschitz: u
  max, min          the largest u among the candidates that lie within their bounds of the winner
  boundary penalty  (d + 3) E relative
The final bound U(x) is the unit: a correct float64 implementation of the definition, in any order, stays within 1 unit.
`judge(value, ref)` = |value - ref.v| / ref.U, with 0 / inf where U = 0.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

E = 2.0 ** -53
C_LIBM = 4.0
EXTENDED = bool(np.finfo(np.longdouble).eps < 2.2e-16)

FIDS = tuple(range(15, 25))
GRID_D = (2, 3, 5, 40, 100, 128)
KINDS = ("inside0", "inside1", "inside2", "near", "nearer", "at_opt", "corner", "corner_mixed", "zero", "peak_tie",
         "wide0", "wide1")
WIDE_BOX = 8.0
_PI_DIGITS = "3.14159265358979323846264338327950288419716939937510"


def grid_instances(d):
    return (0,) if d >= 100 else (0, 1)


# ---- the two arithmetic backends -----------------------------------------------------------------------------------
class _LongDouble:
    name, dtype = "ld", np.longdouble
    log, exp, sin, cos, sqrt, floor, power = np.log, np.exp, np.sin, np.cos, np.sqrt, np.floor, np.power

    @staticmethod
    def num(x):
        return np.longdouble(x) if isinstance(x, str) else np.asarray(x, dtype=np.longdouble)


def _mp_backend(digits=40):
    import mpmath
    mpmath.mp.dps = digits
    lift = np.frompyfunc(lambda v: v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v)), 1, 1)
    B = SimpleNamespace(name="mp", dtype=object)
    B.num = lambda x: mpmath.mpf(x) if isinstance(x, str) else np.asarray(lift(np.asarray(x, dtype=object)), dtype=object)
    for fn in ("log", "exp", "sin", "cos", "sqrt", "floor"):
        setattr(B, fn, (lambda uf: lambda a: np.asarray(uf(a), dtype=object))(np.frompyfunc(getattr(mpmath, fn), 1, 1)))
    pw = np.frompyfunc(mpmath.power, 2, 1)
    B.power = lambda a, p: np.asarray(pw(a, p), dtype=object)
    return B


_B = _LongDouble


def _arr(v):
    return np.asarray(_B.num(v), dtype=_B.dtype)


# ---- value-with-bound arithmetic -----------------------------------------------------------------------------------
class Q:
    __slots__ = ("v", "u")

    def __init__(self, v, u=0.0):
        self.v = _arr(v)
        self.u = _arr(u) + 0 * self.v

    def __getitem__(self, k):
        return Q(self.v[k], self.u[k])

    def __neg__(self):
        return Q(-self.v, self.u)

    def __add__(self, o):
        o = lift(o)
        v = self.v + o.v
        r = np.minimum(E * abs(v), np.minimum(abs(self.v) + self.u, abs(o.v) + o.u))
        return Q(v, self.u + o.u + r)

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-lift(o))

    def __rsub__(self, o):
        return lift(o) + (-self)

    def __mul__(self, o):
        o = lift(o)
        v = self.v * o.v
        r = np.where(_is_pow2(self) | _is_pow2(o), 0, E) * abs(v)
        return Q(v, abs(self.v) * o.u + abs(o.v) * self.u + self.u * o.u + r)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = lift(o)
        v = self.v / o.v
        return Q(v, (self.u + abs(v) * o.u) / abs(o.v) + E * abs(v))

    def __rtruediv__(self, o):
        return lift(o) / self


def _is_pow2(q):
    """An exact factor +-2^k: the product with it is exact."""
    f = np.asarray(q.v, dtype=np.float64)
    return (q.u == 0) & (f == q.v) & (np.abs(np.frexp(f)[0]) == 0.5)


def lift(o):
    """Python numbers are float64 values of the program text: exact."""
    return o if isinstance(o, Q) else Q(_B.num(float(o)) if isinstance(o, (int, float)) else _B.num(o))


def K(text):
    """A decimal constant of the definition: its exact value, bounded by its float64 rounding."""
    v = _B.num(text)
    return Q(v, abs(v - _arr(float(text))))


def two_pi():
    pi = K(_PI_DIGITS)
    return Q(2 * pi.v, 2 * pi.u)                                          # doubling is exact


def qabs(q):
    return Q(abs(q.v), q.u)


def _exact_at(q, point):
    return (q.v == point) & (q.u == 0)


def qlog(q):                                                              # q.v > 0
    v = _B.log(q.v)
    return Q(v, q.u / abs(q.v) + C_LIBM * E * abs(v))


def qexp(q):
    v = _B.exp(q.v)
    return Q(v, v * q.u * (1 + q.u) + np.where(_exact_at(q, 0), 0, C_LIBM * E) * v)


def qsin(q):
    v = _B.sin(q.v)
    return Q(v, (abs(_B.cos(q.v)) + q.u) * q.u + C_LIBM * E * abs(v))


def qcos(q):
    v = _B.cos(q.v)
    return Q(v, (abs(_B.sin(q.v)) + q.u) * q.u + np.where(_exact_at(q, 0), 0, C_LIBM * E) * abs(v))


def qsqrt(q):                                                             # q.v >= 0; sqrt is correctly rounded: C = 1
    v = _B.sqrt(q.v)
    pos = q.v > 0
    slope = q.u / np.where(pos, 2 * v, 1)
    return Q(v, np.where(pos, slope, _B.sqrt(q.u)) + E * v)


def qpow(a, p):
    """a^p for a.v >= 0 and p.v > 0: |p a^(p-1)| u_a + |a^p ln a| u_p + C E a^p; at a = 0 the bound is u_a^p."""
    a, p = lift(a), lift(p)
    pos = a.v > 0
    safe = np.where(pos, a.v, 1)
    v = np.where(pos, _B.power(safe, p.v + 0 * safe), 0 * safe)
    u = abs(p.v) * v / safe * a.u + v * abs(_B.log(safe)) * p.u + np.where(_exact_at(a, 1), 0, C_LIBM * E) * v
    at0 = np.where(a.u > 0, _B.power(np.where(a.u > 0, a.u, 1), p.v + 0 * safe), 0 * safe)
    return Q(v, np.where(pos, u, at0))


def qrelu_sq(q):
    """max(q, 0)^2, as the penalties of f20 write it."""
    m = np.where(q.v > 0, q.v, 0 * q.v)
    v = m * m
    near = q.v + q.u > 0
    return Q(v, np.where(near, 2 * m * q.u + q.u * q.u, 0 * v) + 2 * E * v)


def qsum(q, axis=None):
    n = q.v.size if axis is None else q.v.shape[axis]
    return Q(q.v.sum(axis=axis), q.u.sum(axis=axis) + n * E * abs(q.v).sum(axis=axis))


def qprod(q):
    out = q[0]
    for i in range(1, q.v.shape[0]):
        out = out * q[i]
    return out


def matvec(A, q):
    A = _arr(A)
    d = A.shape[1]
    absA = abs(A)
    return Q(A @ q.v, absA @ q.u + (d + 1) * E * (absA @ abs(q.v)))


def qextreme(q, largest=True):
    s = 1 if largest else -1
    w = int(np.argmax((s * q.v).astype(np.float64)))
    cand = s * q.v + q.u >= s * q.v[w] - q.u[w]
    return Q(q.v[w], np.max(q.u[cand]))


def qselect(cond, a, b):
    a, b = lift(a), lift(b)
    return Q(np.where(cond, a.v, b.v), np.where(cond, a.u, b.u))


# ---- the transformations and the penalty ---------------------------------------------------------------------------
def t_osz(y):
    """T_osz: sign(y) exp(xh + 0.049 (sin(c1 xh) + sin(c2 xh))), xh = log|y|, (c1, c2) = (10, 7.9) for y > 0 and
    (5.5, 3.1) for y < 0, 0 at 0 - in the legacy form t = xh / 0.1, exp(t + 0.49 (sin(k1 t) + sin(k2 t)))^0.1."""
    nz, pos = y.v != 0, y.v > 0
    a = Q(np.where(nz, abs(y.v), 1), np.where(nz, y.u, 0))
    t = qlog(a) / K("0.1")
    s1 = qsin(qselect(pos, t, K("0.55") * t))
    s2 = qsin(qselect(pos, K("0.79"), K("0.31")) * t)
    r = qpow(qexp(t + K("0.49") * (s1 + s2)), K("0.1"))
    sign = np.where(pos, 1, -1)
    # |T_osz'| <= 1.2 around 0 (|T_osz(y)| <= e^0.098 |y|)
    return Q(np.where(nz, sign * r.v, 0 * r.v), np.where(nz, r.u, 1.2 * y.u))


def t_asy(y, beta, mut=()):
    """T_asy^beta: y_i^(1 + beta (i / (D - 1)) sqrt(y_i)) for y_i > 0, y_i otherwise."""
    d = y.v.shape[0]
    pos = y.v > 0
    a = Q(np.where(pos, y.v, 1), np.where(pos, y.u, 0))
    frac = lift(np.arange(d, dtype=np.float64)) / float(d if "asy_over_d" in mut else d - 1)
    r = qpow(a, 1.0 + (lift(beta) * frac) * qsqrt(a))
    return qselect(pos, r, y)


def boundary_penalty(x):
    d = x.shape[0]
    o = np.maximum(abs(_arr(x)) - 5, 0)
    v = (o * o).sum()
    return Q(v, (d + 3) * E * v)


# ---- the ten functions ---------------------------------------------------------------------------------------------
def _f15(x, st, mut):
    d = x.shape[0]
    y = matvec(st.rot_r, lift(x) - lift(st.xopt))
    w = t_osz(t_asy(y, K("0.2"), mut)) if "f15_swap" in mut else t_asy(t_osz(y), K("0.2"), mut)
    z = matvec(st.m, w)
    return 10.0 * (float(d) - qsum(qcos(two_pi() * z))) + qsum(z * z)


def _f16(x, st, mut):
    d = x.shape[0]
    z = matvec(st.m, t_osz(matvec(st.rot_r, lift(x) - lift(st.xopt))))
    ak, bk = lift(0.5 ** np.arange(12)), lift(3.0 ** np.arange(12))
    f0 = qsum(ak * qcos(two_pi() * bk * 0.5))
    zz = z + 0.5
    inner = Q(zz.v[:, None], zz.u[:, None])
    s = qsum(qcos(two_pi() * inner * Q(bk.v[None, :])) * Q(ak.v[None, :]))
    t = s / float(d) - f0
    return 10.0 * (t * t * t) + (10.0 if "f16_pen" in mut else lift(10.0) / float(d)) * boundary_penalty(x)


def _f17(x, st, mut, fid):
    d = x.shape[0]
    m = st.m
    if fid == 18 and "f18_cond" in mut:
        m = (math.sqrt(10.0) ** (np.arange(d) / (d - 1.0)))[:, None] * st.rot_q
    z = matvec(m, t_asy(matvec(st.rot_r, lift(x) - lift(st.xopt)), 0.5, mut))
    last = d - 2 if (fid == 17 and "f17_pairs" in mut) else d - 1
    z0, z1 = z[:last], z[1:last + 1]
    t = z0 * z0 + z1 * z1
    sn = qsin(50.0 * qpow(t, K("0.1")))
    s = qsum(qpow(t, 0.25) * (1.0 + sn * sn)) if last > 0 else lift(0.0)
    t = s / float(d - 1)
    return t * t + (1.0 if (fid == 17 and "f17_pen" in mut) else 10.0) * boundary_penalty(x)


def _f19(x, st, mut):
    d = x.shape[0]
    m = st.m / max(1.0, math.sqrt(d) / 8.0) if "f19_scale" in mut else st.m
    z = matvec(m, lift(x)) + 0.5
    z0, z1 = z[:-1], z[1:]
    c1, c2 = z0 * z0 - z1, 1.0 - z0
    t = 100.0 * (c1 * c1) + c2 * c2
    return 10.0 + 10.0 * qsum(t / 4000.0 - qcos(t)) / float(d - 1)


def _f20(x, st, mut):
    d = x.shape[0]
    xh = lift(2.0 * st.sign * x)                                          # exact: a sign and a factor 2
    off = lift(st.offset)
    zh = Q(xh.v.copy(), xh.u.copy())
    tail = xh[1:] + 0.25 * (xh[:-1] - off[:-1])
    zh.v[1:], zh.u[1:] = tail.v, tail.u
    z = 100.0 * (lift(st.cond) * (zh - off) + off)
    pen = qsum(qrelu_sq(qabs(z) - 500.0))
    tot = qsum(z * qsin(qsqrt(qabs(z))))
    return K("0.01") * (pen + K("418.9828872724339") - tot / float(d))


def _gallagher(x, st, mut, fid):
    d = x.shape[0]
    P = 20 if (fid == 22 and "f22_peaks" in mut) else st.peaks
    tx = matvec(st.rot, lift(x))
    df = Q(tx.v[None, :], tx.u[None, :]) - lift(st.centres[:P])
    e = qsum(lift(st.scales[:P]) * (df * df), axis=1)
    best = qextreme(lift(st.heights[:P]) * qexp((lift(-0.5) / float(d)) * e))
    v = t_osz(10.0 - best)
    return v * v + boundary_penalty(x)


def _f23(x, st, mut):
    d = x.shape[0]
    z = matvec(st.m, lift(x) - lift(st.xopt))
    nterms = 31 if "f23_terms" in mut else 32
    p2 = _arr(2.0 ** np.arange(1, nterms + 1))
    t = z.v[:, None] * p2[None, :]                                         # a power of two: exact
    terms = abs(t - _B.floor(t + _arr(0.5))) / p2[None, :]
    s = Q(terms.sum(axis=1), nterms * z.u + nterms * E * terms.sum(axis=1))
    base = 1.0 + lift(np.arange(1, d + 1, dtype=np.float64)) * s
    p = 10.0 / qpow(float(d), K("1.2"))
    prod = qprod(qpow(base, p))                                            # the definition's form
    via_log = qexp(qsum(p * qlog(base)))                                   # the sum-of-logs form of the same product
    prod = Q(prod.v, np.maximum(prod.u, via_log.u))
    return lift(10.0) / float(d) / float(d) * (prod - 1.0) + boundary_penalty(x)


def _f24(x, st, mut):
    d = x.shape[0]
    mu0 = 2.5
    sfac = 1.0 - 0.5 / (qsqrt(lift(d + 20.0)) - K("4.1"))
    mu1 = -qsqrt((mu0 * mu0 - 1.0) / sfac)
    xh = lift(2.0 * np.where(st.xopt < 0.0, -x, x))
    a, b = xh - mu0, xh - mu1
    s1, s2 = qsum(a * a), qsum(b * b)
    z = matvec(st.rot_r, lift(st.cond) * matvec(st.rot_q, a))
    lo = qextreme(Q(np.stack([s1.v, (float(d) + sfac * s2).v]), np.stack([s1.u, (float(d) + sfac * s2).u])), largest=False)
    return lo + 10.0 * (float(d) - qsum(qcos(two_pi() * z))) + (1e3 if "f24_pen" in mut else 1e4) * boundary_penalty(x)


def evaluate(fid, state, x, mut=(), backend="ld"):
    """The pair (v, U) of function `fid` at the float64 point `x`, from the float64 tables of `state`."""
    global _B
    old, _B = _B, (_LongDouble if backend == "ld" else _mp_backend())
    try:
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            if fid == 15:
                q = _f15(x, state, mut)
            elif fid == 16:
                q = _f16(x, state, mut)
            elif fid in (17, 18):
                q = _f17(x, state, mut, fid)
            elif fid == 19:
                q = _f19(x, state, mut)
            elif fid == 20:
                q = _f20(x, state, mut)
            elif fid in (21, 22):
                q = _gallagher(x, state, mut, fid)
            elif fid == 23:
                q = _f23(x, state, mut)
            elif fid == 24:
                q = _f24(x, state, mut)
            else:
                raise NotImplementedError(fid)
        if backend == "ld":
            return SimpleNamespace(v=np.longdouble(q.v), U=float(q.u))
        return SimpleNamespace(v=q.v.item() if isinstance(q.v, np.ndarray) else q.v, U=float(q.u))
    finally:
        _B = old


def judge(value, ref, extra=0.0):
    """|value - ref.v| in units of ref.U (+ `extra`, an absolute allowance such as E |f| for the f_opt shift)."""
    err = abs(np.longdouble(value) - ref.v)
    unit = ref.U + extra
    if unit == 0:
        return 0.0 if err == 0 else math.inf
    return float(err / np.longdouble(unit))


# ---- mutants: long-double variants that are wrong in one place each ------------------------------------------------
MUTANTS = {                     # name -> (function ids it changes, dimensions at which it differs from the definition)
    "f16_pen": ((16,), None),           # penalty factor 10 for 10 / d
    "f17_pen": ((17,), None),           # factor 1 for 10
    "f24_pen": ((24,), None),           # factor 1e3 for 1e4
    "asy_over_d": ((15, 17, 18), None),  # T_asy with i / d for i / (d - 1)
    "f17_pairs": ((17,), None),         # without the last pair
    "f22_peaks": ((22,), None),         # 20 peaks
    "f23_terms": ((23,), None),         # 31 terms
    "f15_swap": ((15,), None),          # T_asy and T_osz swapped
    "f18_cond": ((18,), None),          # conditioning 10
    "f19_scale": ((19,), (100, 128)),   # without max(1, sqrt(d) / 8): differs where sqrt(d) > 8
}


# ---- the grid ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(fid, inst, d):
    from pcabo.bbob import BBOBProblem
    return BBOBProblem(fid, inst, d)


def _peak_tie(st, d):
    """Midpoint (mapped back by R^T) of the two Gallagher centres whose peak values there are closest."""
    c, h, sc = st.centres, st.heights, st.scales
    ia, ib = np.triu_indices(st.peaks, 1)
    mid = 0.5 * (c[ia] + c[ib])
    va = h[ia] * np.exp((-0.5 / d) * np.sum(sc[ia] * (mid - c[ia]) ** 2, axis=1))
    vb = h[ib] * np.exp((-0.5 / d) * np.sum(sc[ib] * (mid - c[ib]) ** 2, axis=1))
    k = int(np.argmin(np.abs(va - vb)))
    return st.rot.T @ mid[k]


@functools.lru_cache(maxsize=None)
def cases(fid, d):
    """The points of (fid, d): a list of `SimpleNamespace(fid, inst, d, kind, x, wide)`, one seeded generator per (fid, d)."""
    rng = np.random.default_rng([fid, d])
    out = []
    for inst in grid_instances(d):
        p = problem(fid, inst, d)
        xo = p.optimum.x
        pts = [(f"inside{k}", rng.uniform(-5.0, 5.0, d)) for k in range(3)]
        pts.append(("near", np.clip(xo + 1e-3 * rng.normal(size=d), -5.0, 5.0)))
        pts.append(("nearer", np.clip(xo + 1e-9 * rng.normal(size=d), -5.0, 5.0)))
        pts.append(("at_opt", xo.copy()))
        pts.append(("corner", np.full(d, 5.0)))
        pts.append(("corner_mixed", np.where(rng.random(d) < 0.5, -5.0, 5.0)))
        pts.append(("zero", np.zeros(d)))
        if fid in (21, 22):
            tie = _peak_tie(p._state, d)
            if np.all(np.abs(tie) <= 5.0):
                pts.append(("peak_tie", tie))
        for k in range(2):
            w = rng.uniform(-7.0, 7.0, d)
            if not np.any(np.abs(w) > 5.0):
                j = int(rng.integers(d))
                w[j] = math.copysign(5.0 + 2.0 * rng.random(), w[j])
            pts.append((f"wide{k}", w))
        for kind, x in pts:
            x = np.ascontiguousarray(x, dtype=np.float64)
            x.setflags(write=False)
            out.append(SimpleNamespace(fid=fid, inst=inst, d=d, kind=kind, x=x, wide=kind.startswith("wide")))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(fid, d):
    """`[(case, ref)]` of (fid, d), computed once and shared; do not change it."""
    return tuple((c, evaluate(fid, problem(fid, c.inst, d)._state, c.x)) for c in cases(fid, d))


def grid():
    """Every (case, ref) of the grid."""
    for d in GRID_D:
        for fid in FIDS:
            yield from reference(fid, d)
