"""The device-resident L-BFGS-B (csrc/kernels_lbfgsb.hip) branch by branch against its host-stepped twin.

Every case of tests/lbfgsb_cases.py (n = 2 .. 512 over the NP forms, nv = nq k = 1 .. 200 over the lane-tree forms, group sizes
1 .. 5, maxiter 1 .. 3, starts outside the box, cells, ridge boxes, fixed coordinates, flat PI, the variance floor, identical
initial points, the RBF kernel) through one small Batch per GP state, in device mode (PCABO_OPT_DEVICE_LBFGSB = 1) and in twin
mode (2) on the same state and request:

  1. bit equality of candidates, values, info, failed and status; the device's tie count equals the twin's (its evaluation count
     is its nfev again and is compared as such, nothing more; whether the device re-evaluated an end point shows in item 3's
     values = a device evaluation at the candidates);
  2. the twin's branch counters (csrc/lbfgsb.h), united over the table, reach the MUST list of lbfgsb_cases.py - so the branches
     the bit equality has covered are known, on the run that covered them;
  3. properties on the oracle's exact GP, independent of the twin, with the caps this evaluation path is already held to
     (tests/test_gpu_device_lbfgsb.py::test_device_evaluation_against_oracle: value 5e-9, gradient 3e-10 for log-EI and PI;
     tests/test_gpu_ucb.py::_limit("device32") for UCB): candidates inside the box and fixed coordinates on their bound bit for bit,
     end-point values equal to a device evaluation there bit for bit and within the value cap of the oracle, the oracle's projected
     gradient at the end points of groups that ended CONV_PG, no loss against the clamped initial points;
  4. a run inside a batch of three, beside a parked run, and through the begin / end halves equals the same run alone.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

import lbfgsb_cases as LC
from test_gpu_ucb import _limit

pytestmark = pytest.mark.gpu

LOG_EI_PI_CAPS = (5e-9, 3e-10)       # value, gradient: test_device_evaluation_against_oracle's thresholds
PGTOL = 1e-5
CONV_PG = 40
_BATCHES = {}
WORST = {"value": 0.0, "projected_gradient": 0.0, "loss": 0.0}      # measured / allowed, the worst over the cases run


def _caps(case):
    return _limit("device32") if case.acq == "ucb" else LOG_EI_PI_CAPS


def _code(native, case):
    return {"log_ei": native.ACQ_LOG_EI, "pi": native.ACQ_PI, "ucb": native.ACQ_UCB}[case.acq]


def _set_mode(native, bt, mode):
    bt._chk(native.LIB.pcabo_batch_set_option(bt._h, native.OPT_DEVICE_LBFGSB, mode))
    bt.device_lbfgsb = mode


def _conditioned(native, states, kernel):
    """A device-mode Batch of the given (Z, y) states, conditioned."""
    n, k = states[0][0].shape
    bt = native.Batch(len(states), max_n=n, max_d=k, max_q=512, device_lbfgsb=1)
    bt.gp_condition_begin(np.stack([np.asarray(Z) for Z, _ in states]), np.stack([np.asarray(y) for _, y in states]),
                          kernel=native.KERNEL_RBF if kernel == "rbf" else native.KERNEL_MATERN52)
    _, st = bt.gp_wait_eval([np.resize(np.asarray(Z), (64, k)) for Z, _ in states], [float(np.min(y)) for _, y in states])
    assert not st.any(), st
    return bt


def _batch(native, case):
    """One Batch per GP state, shared by the state's cases."""
    if case.state_key not in _BATCHES:
        _BATCHES[case.state_key] = _conditioned(native, [LC.state(case)], case.kernel)
    return _BATCHES[case.state_key]


@pytest.fixture(scope="module", autouse=True)
def _close_batches():
    yield
    for bt in _BATCHES.values():
        bt.close()
    _BATCHES.clear()


@lru_cache(maxsize=None)
def _run_case(name):
    from pcabo import _native as native
    case = LC.BY_NAME[name]
    bt = _batch(native, case)
    ics, box, s, code = LC.initial_points(case), LC.box(case), LC.scalar(case), _code(native, case)
    out = {}
    for mode in (1, 2):
        _set_mode(native, bt, mode)
        res, status = bt.optimize_acqf([ics], [box], [s], case.maximize, code, batch_limit=case.batch_limit, maxiter=case.maxiter)
        # (both calls must have taken the device path: a call that fell back to the host-paced optimiser leaves no record)
        out[mode] = {"res": res[0], "status": int(status[0]),
                     "groups": bt.device_group_out()[0] if mode == 1 else bt.twin_branches()[0]}
    v, g = bt.device_acq_eval([out[1]["res"][0]], [s], case.maximize, code)
    out["eval"] = (v[0], g[0])
    return out


@pytest.mark.parametrize("name", [c.name for c in LC.CASES])
def test_device_takes_the_twins_path_and_ends_where_the_oracle_agrees(native, name):
    torch.set_num_threads(4)
    case = LC.BY_NAME[name]
    r = _run_case(name)
    (cand, vals, info, failed), (tcand, tvals, tinfo, tfailed) = r[1]["res"], r[2]["res"]
    dev, twin = r[1]["groups"], r[2]["groups"]
    # ---- 1. bit equality
    assert r[1]["status"] == r[2]["status"] == 0
    assert np.array_equal(info, tinfo), (name, info, tinfo)
    assert np.array_equal(cand, tcand) and np.array_equal(vals, tvals), name
    assert failed == tfailed
    assert len(dev) == len(twin) == len(case.groups)
    for gi, (d, t) in enumerate(zip(dev, twin)):
        assert (d["niter"], d["nfev"], d["warnflag"], d["task"]) == tuple(int(x) for x in info[gi]), (name, gi, d, info[gi])
        assert d["status"] == 0 and d["evaluation_cap"] == 0, (name, gi, d)
        assert d["evaluations"] == t["evaluations"] and d["ties"] == t["cauchy_ties"], (name, gi, d, t)
    # ---- 3. properties on the oracle
    cap_v, cap_g = _caps(case)
    box = LC.box(case)
    assert (cand >= box[0]).all() and (cand <= box[1]).all(), name
    fixed = range(case.k) if case.fixed == ("all",) else case.fixed
    for c in fixed:
        assert np.array_equal(cand[:, c], np.full(case.num_restarts, box[0][c])), (name, c)
    assert np.array_equal(vals, r["eval"][0]), name
    acq = LC.oracle_acquisition(case)
    ov, og = acq.value_and_grad(cand)
    ov0, _ = acq.value_and_grad(LC.clamped_initial_points(case))
    verr = float((np.abs(vals - ov) / np.maximum(1.0, np.abs(ov))).max())
    worst = {"value": verr / cap_v, "projected_gradient": 0.0, "loss": 0.0}
    for gi, (q0, nq) in enumerate(case.groups):
        sl = slice(q0, q0 + nq)
        if int(info[gi][3]) == CONV_PG:
            g, x = -og[sl], cand[sl]                 # the joint objective is minus the sum of the values
            pg = np.where(g < 0.0, np.maximum(x - box[1], g), np.minimum(x - box[0], g))
            allowed = PGTOL + cap_g * max(1.0, float(np.abs(g).max()))
            worst["projected_gradient"] = max(worst["projected_gradient"], float(np.abs(pg).max()) / allowed)
        allowed = cap_v * float(np.maximum(1.0, np.abs(ov[sl])).sum() + np.maximum(1.0, np.abs(ov0[sl])).sum())
        worst["loss"] = max(worst["loss"], float(ov0[sl].sum() - ov[sl].sum()) / allowed)
    print("[%s] value %.2e of %.1e; measured / allowed: value %.3f, projected gradient %.3f, loss %.3f"
          % (name, verr, cap_v, worst["value"], worst["projected_gradient"], worst["loss"]))
    for key, w in worst.items():
        WORST[key] = max(WORST[key], w)
    assert worst["value"] <= 1.0 and worst["projected_gradient"] <= 1.0 and worst["loss"] <= 1.0, (name, worst)


def test_twin_counters_reach_the_must_list_on_the_device_run(native):
    """The union of the twin's counters over the table, from the same calls the bit equality was asserted on.  The SHOULD list as
    the CPU run established it (tests/test_lbfgsb_branches_cpu.py): update_skipped, formk_skipped, subsm_truncated and cauchy_ties
    reached; cache_hit and ls_failed_restart not reachable with a consistent objective (reported if they are)."""
    rows = []
    for c in LC.CASES:
        tot = dict.fromkeys(native.LBFGSB_BRANCHES, 0)
        for t in _run_case(c.name)[2]["groups"]:
            for nm, v in t.items():
                tot[nm] += v
        rows.append((c.name, tot))
    print("\n[twin of the device L-BFGS-B] case x branch counter\n" + LC.format_table(rows, native.LBFGSB_BRANCHES))
    print("[oracle-side properties, worst measured / allowed over the cases] " + ", ".join("%s %.3f" % kv for kv in WORST.items()))
    reached = {nm: [name for name, br in rows if br[nm]] for nm in native.LBFGSB_BRANCHES}
    for nm in LC.MUST:
        assert reached[nm], nm
    for nm in ("update_skipped", "formk_skipped", "subsm_truncated", "cauchy_ties"):
        assert reached[nm], nm
    # (last bits move events between cases and machines: a counter expected to stay 0 is reported, not asserted)
    for nm in ("cache_hit", "ls_failed_restart") + LC.UNREACHABLE:
        if reached[nm]:
            print("[expected unreached, reached here] %s: %s" % (nm, ", ".join(reached[nm])))


def test_grouping_and_batch_neutrality(native):
    """A run's results in a batch of three, beside a parked run, and through optimize_begin / optimize_end equal the run alone."""
    base = LC.BY_NAME["n65_k13_nv65_logei"]
    cases = [LC.Case("neutral%d" % s, base.n, base.k, seed=s) for s in range(3)]
    states = [LC.state(c) for c in cases]
    args = ([LC.initial_points(c) for c in cases], [LC.box(c) for c in cases], [LC.scalar(c) for c in cases])

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]

    alone = []
    for b in range(3):
        bt = _conditioned(native, [states[b]], base.kernel)
        res, st = bt.optimize_acqf([args[0][b]], [args[1][b]], [args[2][b]])
        assert st[0] == 0
        alone.append(res[0])
        bt.close()
    bt = _conditioned(native, states, base.kernel)
    for mode in (1, 2):
        _set_mode(native, bt, mode)
        res, st = bt.optimize_acqf(*args)
        assert not st.any() and all(same(res[b], alone[b]) for b in range(3)), mode
    _set_mode(native, bt, 1)
    tok = bt.optimize_begin(*args)
    assert tok is not None
    res, st = bt.optimize_end(tok)
    assert not st.any() and all(same(res[b], alone[b]) for b in range(3))
    per_group = bt.device_group_out()
    assert all(g["evaluation_cap"] == 0 and g["evaluations"] == int(res[b][2][gi][1]) for b in range(3) for gi, g in enumerate(per_group[b]))
    bt.set_active([1, 0, 1])
    res, st = bt.optimize_acqf(*args)
    assert st[0] == 0 and st[2] == 0 and st[1] != 0
    assert same(res[0], alone[0]) and same(res[2], alone[2])
    bt.close()
