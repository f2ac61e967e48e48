"""The end points of `optimize_acqf` on the host-paced paths at k > 40 against the extended-precision reference.

The device optimiser stops at k = 40 (`test_gpu_lbfgsb_branches.py` covers it there); beyond it a call steps its
restart groups on the host and evaluates each round by one launch - of the per-query kernels (`k_acq_fused`,
`k_acq_fast`: a plain context) or of `k_acq_group` per restart group (a PCABO_OPT_GROUP_ACQ context).  This is what
every d = 100 iteration does, and its end points were held only by bit hashes and oracle replays at 2e-4 on the
candidates.  Here they are judged by `acq_reference` on the object's OWN conditioned state (`gp_state()`), with nothing
taken from the optimiser but what it returns:

  states   D (50, 41): the smallest k past the device optimiser; n385k65 (385, 65): `k_acq_fused<32>` with three
           contraction trips, `k_acq_group<2>` at k > 40, a group's 5 * 65 and 3 * 65 coordinates as kernel arguments;
           n449k83 (449, 83): `k_acq_group<2>` past 64 KB of LDS, 5 * 83 = 415 of PCABO_QA_MAX = 416 coordinates;
           a round of both groups (10 * 65, 10 * 83 coordinates) goes through the pointer on the plain context
  scalars  log-EI at the incumbent `near` of `acq_reference.cases`, UCB at kappa = sqrt 2, both minimising
  call     10 initial points, batch_limit 5 (two groups of five) and 3 (3 + 3 + 3 + 1), the state's search box with one
           coordinate fixed (lo = hi), two of the starts outside the box

  1. candidates inside the box, the fixed coordinate on its bound bit for bit;
  2. `vals` within 16 units of the reference's value at `cand` and within FAMILIES_UNITS of `acq_eval(cand)` on the
     same context;
  3. for every group that ended on the projected gradient (task 40, LBFGSB_CONV_PG): the REFERENCE's projected gradient
     at the end points (the formula of `test_gpu_lbfgsb_branches.py` item 3) at most PGTOL = 1e-5 (scipy's value, the
     library's) plus 16 times the largest gradient unit of the group - the optimiser stopped on a device gradient that
     is within 16 units of the reference's in every component, and the projection moves no component further apart;
  4. per group, the reference's summed value at `cand` is not below that at the clamped initial points by more than 16
     times the summed value units of both - the line search accepts no point whose device value is worse;
  5. at least one group per state ends on task 40, so that item 3 has run: if none does the test fails and says so
     (the FIT_STATES rule of `test_gpu_mll_edges.py`).
"""
import math
import time

import numpy as np
import pytest

import acq_reference as A
from test_gpu_acq_edges import FAMILIES_UNITS, LIMIT

pytestmark = pytest.mark.gpu

STATES = ("D", "n385k65", "n449k83")
PGTOL = 1e-5
CONV_PG = 40
NUM_RESTARTS = 10
BATCH_LIMITS = (5, 3)
OUTSIDE = (1, 7)                     # the starts that lie outside the box: one in each group of five, in groups 0 and 2 of 3
FIXED = 1                            # the coordinate with lo = hi


def box_and_starts(st):
    """(2 x k box, 10 x k initial points): the state's search box with coordinate FIXED pinned to its middle; eight
    starts half a lengthscale (in normalised units: the training points span [0, 1]) off seeded training points - where
    the acquisition has structure, so that a run ends on its gradient - and two uniform in the box; of those ten, the
    starts OUTSIDE are moved out of the box: the first by 30 % of the width above it in every even coordinate, the
    second below it in every third."""
    box = A.search_box(st.Z)
    mid = 0.5 * (box[0][FIXED] + box[1][FIXED])
    box[0][FIXED] = box[1][FIXED] = mid
    rng = np.random.default_rng(7000 + 10 * st.n + st.k)
    width = box[1] - box[0]
    span = st.Z.max(axis=0) - st.Z.min(axis=0)
    ics = rng.uniform(box[0], box[1], size=(NUM_RESTARTS, st.k))
    near = rng.choice(st.n, size=8, replace=False)
    ics[[0, 2, 3, 4, 5, 6, 8, 9]] = st.Z[near] + 0.5 * st.lengthscale / math.sqrt(st.k) * span * rng.normal(size=(8, st.k))
    ics[OUTSIDE[0], 0::2] = box[1][0::2] + 0.3 * width[0::2]
    ics[OUTSIDE[1], 0::3] = box[0][0::3] - 0.3 * width[0::3]
    return box, ics


def scalars_of(lin):
    """[(label, acq, maximize, scalar)]: log-EI at `near`, UCB at kappa = sqrt 2, minimising."""
    near = {label: c for label, *c in A.cases(lin)}["log_ei,0,near"]
    return [("log_ei,0,near", A.LOG_EI, 0, near[2]), ("ucb,0,sqrt2", A.UCB, 0, math.sqrt(2.0))]


def projected_gradient(g, x, box):
    """scipy's projgr of the objective's gradient g at x (test_gpu_lbfgsb_branches.py item 3)."""
    return np.where(g < 0.0, np.maximum(x - box[1], g), np.minimum(x - box[0], g))


@pytest.mark.parametrize("name", STATES)
def test_end_points_of_the_host_paced_optimiser_against_the_reference(native, name, capsys):
    t0 = time.time()
    st, _, _ = A.prepared(name)
    n, k = st.n, st.k
    assert k > 40                                                              # beyond the device optimiser
    box, ics = box_and_starts(st)
    x0 = np.clip(ics, box[0], box[1])
    for j in OUTSIDE:
        assert not ((ics[j] >= box[0]) & (ics[j] <= box[1])).all()
    assert box[0][FIXED] == box[1][FIXED] and (np.delete(box[1] - box[0], FIXED) > 0.0).all()
    kcode = native.KERNEL_RBF if st.kernel == "rbf" else native.KERNEL_MATERN52
    codes = {A.LOG_EI: native.ACQ_LOG_EI, A.UCB: native.ACQ_UCB}
    ctxs = {"plain": native.Context(max_n=n, max_d=k, max_q=512), "group": native.Context(max_n=n, max_d=k, max_q=512)}
    ctxs["group"].set_option(native.OPT_GROUP_ACQ, 1)
    rows, fails, converged = [], [], 0
    try:
        for tag, c in ctxs.items():
            c.set_option(native.OPT_BESTF_F32, 0)
            c.gp_condition(st.y, Z=st.Z, norm_bounds=st.norm_bounds, lengthscale=st.lengthscale, noise=st.noise, kernel=kcode)
            gs = c.gp_state()
            _, lin130 = A.cached_linear(st, gs)
            for label, acq, mx, s in scalars_of(lin130):
                for bl in BATCH_LIMITS:
                    cand, vals, info, _ = c.optimize_acqf(ics, box, s, bool(mx), codes[acq], batch_limit=bl)
                    dv, _ = c.acq_eval(cand, s, bool(mx), codes[acq])
                    ref = A.scalars(A.linear(st, gs, np.vstack([cand, x0])), s, mx, acq)       # rows 0 .. 9: cand, 10 .. 19: x0
                    end = slice(0, NUM_RESTARTS)
                    case = (tag, label, bl)
                    # 1. the box
                    if not ((cand >= box[0]).all() and (cand <= box[1]).all()):
                        fails.append((case, "a candidate outside the box"))
                    if not np.array_equal(cand[:, FIXED], np.full(NUM_RESTARTS, box[0][FIXED])):
                        fails.append((case, "the fixed coordinate left its bound"))
                    # 2. the values
                    r_val, _ = A.judge(ref, vals, rows=end)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        r_eval = float(np.nan_to_num(np.abs(vals - dv) / ref.u_value[end], nan=np.inf).max())
                    if not r_val <= LIMIT:
                        fails.append((case, "vals against the reference", r_val))
                    if not r_eval <= FAMILIES_UNITS:
                        fails.append((case, "vals against acq_eval(cand)", r_eval))
                    # 3. and 4. per group
                    r_pg, r_loss, tasks = 0.0, -math.inf, []         # (a negative loss: the group gained)
                    groups = [(g0, min(bl, NUM_RESTARTS - g0)) for g0 in range(0, NUM_RESTARTS, bl)]
                    assert len(groups) == len(info)
                    for (g0, nq), row in zip(groups, info):
                        sl, sl0 = slice(g0, g0 + nq), slice(NUM_RESTARTS + g0, NUM_RESTARTS + g0 + nq)
                        tasks.append(int(row[3]))
                        if int(row[3]) == CONV_PG:
                            converged += 1
                            g = -A.f64(ref.grad[sl])                           # the joint objective is minus the sum of the values
                            pg = float(np.abs(projected_gradient(g, cand[sl], box)).max())
                            r_pg = max(r_pg, pg / (PGTOL + LIMIT * float(ref.u_grad[sl].max())))
                        loss = float(A.f64(ref.value[sl0].sum() - ref.value[sl].sum()))
                        r_loss = max(r_loss, loss / (LIMIT * float(ref.u_value[sl].sum() + ref.u_value[sl0].sum())))
                    if not r_pg <= 1.0:
                        fails.append((case, "the reference's projected gradient at a CONV_PG end", r_pg))
                    if not r_loss <= 1.0:
                        fails.append((case, "the end points lose against the clamped initial points", r_loss))
                    rows.append("  %-5s %-14s batch_limit %d: value %.2g / %g units, against acq_eval %.2g / %g units; "
                                "measured / allowed: projected gradient %.3g, loss %.3g; tasks %s, iterations %s"
                                % (tag, label, bl, r_val, LIMIT, r_eval, FAMILIES_UNITS, r_pg, r_loss, tasks,
                                   [int(r[0]) for r in info]))
    finally:
        for c in ctxs.values():
            c.close()
    with capsys.disabled():
        print("\n[optimize_acqf end points, state %s (n=%d k=%d), %d groups ended on the projected gradient; %.1f s]\n%s"
              % (name, n, k, converged, time.time() - t0, "\n".join(rows)))
    assert not fails, (len(fails), fails[:12])
    assert converged, ("no group of state %s ends on the projected-gradient stop (task 40): the check of the reference's "
                       "projected gradient did not run, choose other starts" % name)
