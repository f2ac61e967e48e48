"""The device BBOB objectives (`k_bbob_eval`, csrc/kernels_bbob.hip) against an extended-precision reference at edge shapes.

Every value is judged in the unit of `bbob_reference` - a first-order worst-case bound on the error of any float64
evaluation of the definition, none of it taken from a run of the kernel - and the limit is 1 unit on every case of the
grid: d = 2 (one pair, i / (d - 1) is 0 or 1) to d = 128 = PCABO_MAXD (LDS vectors full, largest table), points at, next to
and far from x_opt, the corners of the box, the origin, a point between two Gallagher peaks, and points beyond |x| = 5 in a
wider box, where the in-kernel boundary penalty runs.  `test_bbob_reference_cpu.py` proves the reference itself and shows
that one wrong factor, index range or transform leaves the unit by >= 1e5.  The out-of-box rule, the independence of a
run's value from its slot in the batch and the argument refusals of the C interface are checked exactly.
"""
import ctypes as C
import math

import numpy as np
import pytest

import bbob_reference as br

pytestmark = pytest.mark.gpu

PENALTY = 1000.0
ERR_ARG = -1


def _problems(d):
    return [br.problem(fid, inst, d) for fid in br.FIDS for inst in br.grid_instances(d)]


@pytest.fixture(scope="module")
def objectives(native):
    """One `DeviceObjectives` per dimension over all functions and instances of the grid, built on first use."""
    from pcabo.bbob_device import DeviceObjectives
    made = {}

    def get(d):
        if d not in made:
            made[d] = DeviceObjectives(_problems(d), penalty=PENALTY)
        return made[d]

    yield get
    for dev in made.values():
        dev.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.mark.parametrize("d", br.GRID_D)
def test_values_within_one_unit(objectives, d):
    """raw[b] and f[b] - f_opt of every case of the grid, one `evaluate` per case kind: <= 1 unit, no case left out.
    Measured on an MI355X, worst units per function over the grid: f15 0.21, f16 0.66, f17 0.87, f18 0.81, f19 0.27,
    f20 0.61, f21 0.81, f22 0.74, f23 0.51, f24 0.21 (EXPERIMENTS.md section 29; the host restatement 0.13 ... 0.38)."""
    dev = objectives(d)
    probs = dev.problems
    assert dev.B == (10 if d >= 100 else 20)
    by_row = [{c.kind: (c, ref) for c, ref in br.reference(int(p.meta_data.problem_id), d)
               if c.inst == int(p.meta_data.instance)} for p in probs]
    worst, bad, judged = {}, [], 0
    for kind in br.KINDS:
        rows = [b for b in range(dev.B) if kind in by_row[b]]
        if not rows:
            continue
        wide = kind.startswith("wide")
        X = np.stack([by_row[b][kind if kind in by_row[b] else "inside0"][0].x for b in range(dev.B)])
        box = br.WIDE_BOX if wide else 5.0
        dev.lb, dev.ub = -box, box
        try:
            f, raw, oob = dev.evaluate(X)
        finally:
            dev.lb, dev.ub = -5.0, 5.0
        assert not oob.any(), (d, kind, oob)
        for b in rows:
            c, ref = by_row[b][kind]
            assert wide == bool(np.any(np.abs(c.x) > 5.0))
            j_raw = br.judge(raw[b], ref)
            shifted = np.longdouble(f[b]) - np.longdouble(probs[b].f_opt)
            j_f = br.judge(shifted, ref, extra=br.E * abs(f[b]))
            judged += 1
            j = max(j_raw, j_f)
            if j >= worst.get(c.fid, (0.0, None))[0]:
                worst[c.fid] = (j, f"{kind}/i{c.inst}")
            if not (j_raw <= 1.0 and j_f <= 1.0):
                bad.append((c.fid, c.inst, d, kind, j_raw, j_f, raw[b], float(ref.v), ref.U))
    for fid in br.FIDS:
        print(f"device f{fid} d={d}: worst {worst[fid][0]:.3g} units at {worst[fid][1]}")
    assert judged == sum(len(r) for r in by_row) and judged >= 11 * dev.B
    assert not bad, bad


def _host_outside(x, lb=-5.0, ub=5.0):
    """The rule of pcabo/batchrun.py, as written there: a NaN is outside."""
    return bool(not np.all(x >= lb) or not np.all(x <= ub))


@pytest.mark.parametrize("d", br.GRID_D)
def test_out_of_the_box(objectives, d):
    """5 + ulp, -5 - ulp, 1e30, -1e308, +-inf and nan on coordinate 0, d // 2 and d - 1 of an otherwise inside point: oob,
    raw == f == penalty exactly, the inside rows of the same call keep their bits, +-5 exactly are inside, and the host
    rule of batchrun.py gives the same verdict on every row."""
    dev = objectives(d)
    B = dev.B
    base = np.stack([br.cases(int(p.meta_data.problem_id), d)[0].x for p in dev.problems])
    assert not any(_host_outside(x) for x in base)
    f0, raw0, oob0 = dev.evaluate(base)
    assert not oob0.any()
    values = [np.nextafter(5.0, np.inf), np.nextafter(-5.0, -np.inf), 1e30, -1e308, np.inf, -np.inf, np.nan]
    places = [(v, i) for i in (0, d // 2, d - 1) for v in values]
    per_call = B // 2
    for start in range(0, len(places), per_call):
        X = base.copy()
        hit = {}
        for k, (v, i) in enumerate(places[start:start + per_call]):
            b = (2 * k + 1 + 2 * (start // per_call)) % B                 # odd rows (B is even), shifted call by call
            X[b, i] = v
            hit[b] = (v, i)
        assert len(hit) == len(places[start:start + per_call])
        f, raw, oob = dev.evaluate(X)
        for b in range(B):
            assert bool(oob[b]) == _host_outside(X[b]) == (b in hit), (d, b, hit.get(b))
            if b in hit:
                assert raw[b] == PENALTY and f[b] == PENALTY, (d, b, hit[b], raw[b], f[b])
            else:
                assert _bits(raw[b]) == _bits(raw0[b]) and _bits(f[b]) == _bits(f0[b]), (d, b)
    # +-5 exactly: inside, evaluated
    X = base.copy()
    edge = {}
    for k, (v, i) in enumerate((v, i) for i in (0, d // 2, d - 1) for v in (5.0, -5.0)):
        X[k, i] = v
        edge[k] = (v, i)
    f, raw, oob = dev.evaluate(X)
    assert not oob.any() and not any(_host_outside(x) for x in X)
    for b in range(B):
        if b in edge:
            assert np.isfinite(raw[b]) and f[b] == raw[b] + dev.f_opt[b]
        else:
            assert _bits(raw[b]) == _bits(raw0[b])


@pytest.mark.parametrize("d", (5, 128))
def test_value_is_independent_of_slot_and_neighbours(native, d):
    """One work-group per run, no state across them: a problem alone (B = 1) returns the bits it returns in slot 0, in a
    middle slot and in the last slot of a B = 30 batch of mixed functions; two calls of one batch return the same bytes."""
    from pcabo.bbob_device import DeviceObjectives
    rng = np.random.default_rng([77, d])
    B = 30
    for fid in br.FIDS:
        target = br.problem(fid, 0, d)
        x = br.cases(fid, d)[0].x
        alone = DeviceObjectives([target], penalty=PENALTY)
        f1, raw1, oob1 = alone.evaluate(x[None, :])
        f1b, raw1b, _ = alone.evaluate(x[None, :])
        alone.close()
        assert _bits(raw1) == _bits(raw1b) and _bits(f1) == _bits(f1b) and not oob1[0]
        slots = (0, B // 2, B - 1)
        others = [br.FIDS[(fid - 15 + 1 + k) % 10] for k in range(B)]       # every other function next to the target
        probs = [target if b in slots else br.problem(others[b], 0, d) for b in range(B)]
        X = rng.uniform(-5.0, 5.0, (B, d))
        X[1, 0] = 7.0                                                       # an outside neighbour as well
        for b in slots:
            X[b] = x
        batch = DeviceObjectives(probs, penalty=PENALTY)
        fa, rawa, ooba = batch.evaluate(X)
        fb, rawb, oobb = batch.evaluate(X)
        batch.close()
        assert _bits(rawa) == _bits(rawb) and _bits(fa) == _bits(fb) and np.array_equal(ooba, oobb)
        assert ooba[1] and not ooba[list(slots)].any()
        for b in slots:
            assert _bits(rawa[b]) == _bits(raw1[0]) and _bits(fa[b]) == _bits(f1[0]), (fid, d, b, rawa[b], raw1[0])


def _lib(native):
    lib = native.LIB
    lib.pcabo_bbob_table_doubles.argtypes = [C.c_int]
    lib.pcabo_bbob_table_doubles.restype = C.c_int
    lib.pcabo_bbob_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.pcabo_bbob_create.restype = C.c_int
    lib.pcabo_bbob_destroy.argtypes = [C.c_void_p]
    lib.pcabo_bbob_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.pcabo_bbob_eval.restype = C.c_int
    return lib


def test_argument_refusals(native):
    """The argument checks of pcabo_bbob_table_doubles / _create / _eval: PCABO_ERR_ARG, `*out` left null, nothing launched."""
    lib = _lib(native)
    for d in (1, 129, 0, -3):
        assert lib.pcabo_bbob_table_doubles(d) == ERR_ARG
    for d in (2, 128):                              # [x_opt(d) | R(d*d) | M(d*d) | aux(101*(2d+1) + 4d + 8)]
        assert lib.pcabo_bbob_table_doubles(d) == d + 2 * d * d + 101 * (2 * d + 1) + 4 * d + 8

    def create(B, d, fid, tables=True, out=True):
        stride = max(lib.pcabo_bbob_table_doubles(min(max(d, 2), 128)), 1)
        t = np.zeros(max(B, 1) * stride)
        ids = None if fid is None else np.asarray(fid, dtype=np.int32)
        h = C.c_void_p(0xdead)                      # must come back null
        rc = lib.pcabo_bbob_create(0, B, d, None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                   t.ctypes.data_as(C.c_void_p) if tables else None, C.byref(h) if out else None)
        return rc, h.value

    for args in ((0, 5, []), (3, 1, [15, 16, 17]), (3, 129, [15, 16, 17]), (3, 5, [14, 16, 17]), (3, 5, [15, 14, 17]),
                 (3, 5, [15, 16, 14]), (3, 5, [25, 16, 17]), (3, 5, [15, 25, 17]), (3, 5, [15, 16, 25]), (3, 5, None)):
        rc, h = create(*args)
        assert rc == ERR_ARG and h is None, (args, rc, h)
    rc, h = create(3, 5, [15, 16, 17], tables=False)
    assert rc == ERR_ARG and h is None
    rc, h = create(3, 5, [15, 16, 17], out=False)
    assert rc == ERR_ARG

    # eval: null handle, null X, null raw refused; a null oob accepted
    p = br.problem(15, 0, 2)
    from pcabo.bbob_device import _table
    stride = lib.pcabo_bbob_table_doubles(2)
    t = _table(p, stride)
    ids = np.array([15], dtype=np.int32)
    h = C.c_void_p()
    assert lib.pcabo_bbob_create(0, 1, 2, ids.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), C.byref(h)) == 0
    try:
        x = np.array([[1.0, -2.0]])
        raw, oob = np.full(1, math.nan), np.full(1, -7, dtype=np.int32)
        px, pr, po = (a.ctypes.data_as(C.c_void_p) for a in (x, raw, oob))
        assert lib.pcabo_bbob_eval(None, px, -5.0, 5.0, PENALTY, pr, po) == ERR_ARG
        assert lib.pcabo_bbob_eval(h, None, -5.0, 5.0, PENALTY, pr, po) == ERR_ARG
        assert lib.pcabo_bbob_eval(h, px, -5.0, 5.0, PENALTY, None, po) == ERR_ARG
        assert math.isnan(raw[0]) and oob[0] == -7                         # the refusals wrote nothing
        assert lib.pcabo_bbob_eval(h, px, -5.0, 5.0, PENALTY, pr, None) == 0
        ref = br.evaluate(15, p._state, x[0])
        assert br.judge(raw[0], ref) <= 1.0 and oob[0] == -7
        assert lib.pcabo_bbob_eval(h, px, -5.0, 5.0, PENALTY, pr, po) == 0 and oob[0] == 0
    finally:
        lib.pcabo_bbob_destroy(h)
