"""The host L-BFGS-B (csrc/lbfgsb.cpp) branch by branch, on the oracle alone - no GPU.

Every case of tests/lbfgsb_cases.py with n <= 130: the oracle's exact GP and its acquisition (log-EI, PI, UCB), botorch's joint
objective -(sum of the values) per restart group, as test_lbfgsb_vs_scipy.py::test_joint_five_restart_acquisition_problem_same_path_as_scipy.

  * Summation order 0 against scipy's own L-BFGS-B with the same maxiter, every group of every case: (nit, nfev) and warnflag equal,
    x within 1e-8, and the first 10 evaluated points within 1e-8 of scipy's - the scipy pin on active-set, fixed-variable and
    tiny-maxiter acquisition problems.  One long group is exempt from the end-point bound, by name
    (lbfgsb_cases.SCIPY_END_POINT_EXEMPT: scipy's counts after 107 evaluations, end points 2.7e-6 apart): the two implementations
    round their sums in different orders and L-BFGS-B amplifies the last bit (tests/test_lbfgsb_divergence.py).
  * Summation order 1 (the device optimiser's twin): the branch counters of lbfgsb.h, summed over a case's groups.  Every counter of
    the MUST list is reached by at least two cases; the case x counter table is printed (-s).

The SHOULD list on this surface:
  reached:  update_skipped, formk_skipped, subsm_truncated, cauchy_ties (two identical initial points in one group).
  cache_hit: not reached.  The driver reuses the last evaluation when a trial point repeats it bit for bit, which takes a line search
    that shrinks its step until x + stp d == x.  Tried: the variance-floor state (n30_k3_floor_logei), PI from its exactly flat
    plateau (n*_flat_pi: the start already has a zero gradient), cells of 1e-3 of the box and maxiter 1 .. 3.  With a value and a
    gradient that agree, dcsrch accepts a step within a few trials (ls_backtracked never needs more than a handful); only an
    objective whose value contradicts its gradient gets there (test_abnormal_line_search_and_memoised_repeats_like_scipy).
  ls_failed_restart: not reached, for the same reason - it takes 20 backtracks or an ascent direction with a history present.
The failure resets reset_after_cauchy / _subsm / _formt, ls_ascent and abnormal are unreachable with a consistent objective (a
factorisation of the compact matrices fails, or the direction is no descent direction); the test reports any that is reached.  reset_after_formk
was expected among them and IS reached, by the single-restart groups in narrow ridge boxes (n*_x32_*: formk's second Cholesky
factorisation fails on a two- or three-variable problem, the memory is dropped and the iteration starts again) - with scipy's
counts and end points, so the reset is scipy's too.
ABNORMAL on the host is test_lbfgsb_vs_scipy.py::test_abnormal_line_search_and_memoised_repeats_like_scipy.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch
from scipy.optimize import minimize

import lbfgsb_cases as LC

SHOULD_REACHED = ("update_skipped", "formk_skipped", "subsm_truncated", "cauchy_ties")


@lru_cache(maxsize=None)
def _run_case(name):
    """Per restart group of the case: scipy's result, this library's in the published order, the tree order's branch counters."""
    from pcabo import _native as native
    torch.set_num_threads(1)
    case = LC.BY_NAME[name]
    acq = LC.oracle_acquisition(case)
    out = []
    for q0, nq in case.groups:
        x0, bounds = LC.group_problem(case, q0, nq)
        fun = LC.joint_objective(acq, nq, case.k)
        seen = {"scipy": [], "cpp": []}

        def recording(tag):
            def rec(x):
                seen[tag].append(np.array(x, dtype=np.float64, copy=True))
                return fun(x)
            return rec
        ref = minimize(recording("scipy"), x0, jac=True, method="L-BFGS-B", bounds=bounds, options={"maxiter": case.maxiter})
        mine = native.lbfgsb_minimize(recording("cpp"), x0, bounds, maxiter=case.maxiter)
        was = native.lbfgsb_set_sum_order(1)
        try:
            tree = native.lbfgsb_minimize(fun, x0, bounds, maxiter=case.maxiter)
        finally:
            native.lbfgsb_set_sum_order(was)
        out.append({"q0": q0, "ref": ref, "mine": mine, "tree": tree, "seen": seen})
    return out


def _case_counters(name):
    tot = {}
    for g in _run_case(name):
        for nm, v in g["tree"]["branches"].items():
            tot[nm] = tot.get(nm, 0) + v
    return tot


@pytest.mark.parametrize("name", [c.name for c in LC.CPU_CASES])
def test_published_order_takes_scipys_path(native, name):
    for g in _run_case(name):
        ref, mine = g["ref"], g["mine"]
        # (all variables fixed: scipy answers without calling its L-BFGS-B - one evaluation, no iteration count)
        got = (mine["nit"], mine["nfev"], mine["warnflag"])
        want = (int(getattr(ref, "nit", 0)), int(ref.nfev), 0 if ref.success else (1 if ref.status == 1 else 2))
        dx = float(np.abs(ref.x - mine["x"]).max())
        xs, xc = g["seen"]["scipy"][:LC.SCIPY_PREFIX], g["seen"]["cpp"][:LC.SCIPY_PREFIX]
        head = max(float(np.abs(a - c).max()) for a, c in zip(xs, xc))
        print("[%s group at %d] scipy nit/nfev/warnflag %s, lbfgsb.cpp %s, |dx| %.2e; first %d evaluated points %.2e"
              % (name, g["q0"], want, got, dx, len(xs), head))
        assert len(xs) == len(xc) and head < 1e-8, (name, g["q0"], len(xs), len(xc), head)
        assert mine["branches"]["evaluations"] == mine["nfev"]
        assert got == want, (name, g["q0"], got, want)
        if (name, g["q0"]) in LC.SCIPY_END_POINT_EXEMPT:
            assert want[1] > LC.SCIPY_LONG, (name, g["q0"], want)      # only a long run may be on the list
        else:
            assert dx < 1e-8, (name, g["q0"], dx)


def test_tree_order_reaches_every_branch_of_the_must_list(native):
    rows = [(c.name, _case_counters(c.name)) for c in LC.CPU_CASES]
    print("\n[host L-BFGS-B, tree order, oracle surface] case x branch counter\n" + LC.format_table(rows, native.LBFGSB_BRANCHES))
    assert set(LC.MUST) | set(LC.SHOULD) | set(LC.ALSO_REACHED) | set(LC.UNREACHABLE) | {"evaluations"} == set(native.LBFGSB_BRANCHES)
    reached = {nm: [name for name, br in rows if br[nm]] for nm in native.LBFGSB_BRANCHES}
    for nm in LC.MUST:
        assert len(reached[nm]) >= 2, (nm, reached[nm])
    for nm in SHOULD_REACHED + LC.ALSO_REACHED:
        assert len(reached[nm]) >= 1, nm
    # (last bits move events between cases and machines: a counter expected to stay 0 is reported, not asserted)
    for nm in ("cache_hit", "ls_failed_restart") + LC.UNREACHABLE:
        if reached[nm]:
            print("[expected unreached, reached here] %s: %s" % (nm, ", ".join(reached[nm])))
    # the tree order takes scipy's counts on these problems too, wherever the run is short (the orders part in the last bits)
    for c in LC.CPU_CASES:
        if c.maxiter <= 3:
            for g in _run_case(c.name):
                assert (g["tree"]["nit"], g["tree"]["nfev"]) == (g["mine"]["nit"], g["mine"]["nfev"]), c.name
