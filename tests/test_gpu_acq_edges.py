"""log-EI and PI on every evaluation path of the device against an extended-precision reference at edge shapes.

The acquisition kernels - `k_acq_fast<SLAB, NB>`, `k_acq_fused`, `k_acq_group`, `k_acq_combine`, the GEMM scoring
(`k_score_ks`, `k_score_mu`, `k_score_gemm`) and `lb_eval` of `k_lbfgsb_group`, all on the scalar maths of acq_math.h -
are judged in the error units of `acq_reference` (first-order analysis of any fp64 implementation of the chain;
`test_acq_reference_cpu.py` shows a numpy restatement staying under 4 of each and wrong variants leaving them).  The
device sums in other orders (slabs, wave reductions, MFMA chains), so its constants may differ by small factors: the
acceptance limit is 16 in every unit, as in `test_gpu_gp_edges.py` and `test_gpu_wpca_edges.py`.

The reference starts from each object's OWN conditioned state (`gp_state()` of the context, of the group context, of
the batch's run), read once after conditioning and taken as exact: the conditioning is judged by `test_gpu_gp_edges.py`,
and its kappa-type factors stay out of the units here.

Four of the states lie in the stress region of the d = 100 runs (n = 300 .. 1050, k ~ 85; the arithmetic is beside each
state in `acq_reference.STATES`): n385k65 - `k_acq_fused<32>` with k > 32 (three trips of its gradient contraction, the
second trip of `acq_tail`'s and `acq_finish_query`'s component loops, the `c != l` side of `acq_tail`'s bounds) and
`k_acq_group<2>` at k > 40; n449k83 - `k_acq_group<2>` with more than 64 KB of dynamic LDS and 415 of the 416 argument
coordinates; n1025 - `k_acq_group<5>` with all five columns per thread live, `k_acq_combine` over 34 records, five
`k_score_ks` blocks and 17 row blocks of `k_score_gemm`; n1473 - the second iteration of `grad_partial_sum`'s unrolled
loop (48 slabs), six `k_score_ks` blocks, and the group context beyond `acq_group_possible`, whose results must be the
plain context's bit for bit (GROUP_TWINS).

The entry points and their order are those of `test_gpu_ucb.py`; the incumbents are float64 (`PCABO_OPT_BESTF_F32`
off, as for a numpy float64 incumbent), because the seam incumbents must put u at -1 and -1e6 to rounding.
"""
import time

import numpy as np
import pytest

import acq_reference as A

pytestmark = pytest.mark.gpu

LIMIT = 16.0
FAMILIES_AGREE = 1e-10                 # the kernel families on the same factor (tests/test_gpu_ucb.py)
# Where the families are held to it: every VALUE of every scalar, and every GRADIENT but those of queries deep in the
# middle branch of `log_ei_helper` under the incumbents that send queries there (log-EI `mid`, `seam-1e6`).  There each
# evaluation of h' = -u - w'(u) E / (1 - E) carries 5 eps |u|^3 of rounding noise (the cancellation of w'(u), botorch's
# own: u_dh of acq_reference; test_acq_reference_cpu.py prints it, 2e-8 relative at |u| ~ 1e3, 4e-4 at 1e5), so two
# evaluations cannot agree to 1e-10 beyond |u| ~ 67.  Under those incumbents the gradients agree to 1e-10 at the queries
# `acq_reference.well_conditioned` names from the reference's u, and at ALL queries every component of two families
# lies within FAMILIES_UNITS of the reference's own unit - the unit that carries the 5 eps |u|^3.  The values are not
# amplified (a last-bit change of u moves u^2 / 2 by 2 du / |u| relative).
DEEP_MIDDLE = ("mid", "seam-1e6")
FAMILIES_UNITS = 2.0 * LIMIT           # two results within LIMIT units of the reference are this close to each other
PATHS = ("q5", "q6", "finish32", "combine40", "fast130", "gemm130", "group5", "group6", "group32", "group40",
         "group130", "groupgemm130", "batch130", "device32")


# Beyond `acq_group_possible` (kernels_acq.hip: NP <= 1280 and k <= 128; state n1473 has NP = 1536) a
# PCABO_OPT_GROUP_ACQ context cannot take k_acq_group: `group_mode` (pcabo_api.hip) is false and `pcabo_acq_eval` goes
# through `eval_staged`, the plain context's per-query launches, with the same arguments.  Its results are then the plain
# context's BIT FOR BIT, path by path - a stronger statement than the families rule, which stays for every other state.
GROUP_TWINS = (("group5", "q5"), ("group6", "q6"), ("group32", "finish32"), ("group40", "combine40"),
               ("group130", "fast130"), ("groupgemm130", "gemm130"))


def group_kernel_possible(n, k):
    """`acq_group_possible` of kernels_acq.hip at the padded size of n points."""
    return 64 * -(-n // 64) <= 1280 and k <= 128


def _verr(v, ov):
    return float((np.abs(v - ov) / np.maximum(1.0, np.abs(ov))).max())


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))


@pytest.mark.parametrize("name", list(A.STATES))
def test_log_ei_and_pi_against_the_reference_on_every_path(native, name, capsys):
    """Per state, direction and scalar (log-EI at near / mid / far and at the three seam incumbents, PI at near /
    3sigma): every value and every gradient component of
      q5, q6, finish32, combine40   Context.acq_eval: a whole group, a partial group, the in-launch finish, records + k_acq_combine
      fast130                       Context.acq_eval at q = 130 with gradients: 8 queries per work-group on the fast path
      gemm130                       gp_wait_eval at q = 130: GEMM scoring with partial 64-tiles
      group*                        the same on a PCABO_OPT_GROUP_ACQ context (k_acq_group up to q = 32)
      batch130                      Batch.gp_wait_eval: the batched scoring launch
      device32                      Batch(device_lbfgsb=1).device_acq_eval: lb_eval (k <= 40 and n <= 512)
    within 16 units of the reference on the object's own state.  Prints the worst ratio per path."""
    t0 = time.time()
    st, _, _ = A.prepared(name)
    n, k, Z, y, X = st.n, st.k, st.Z, st.y, st.X
    kcode = native.KERNEL_RBF if st.kernel == "rbf" else native.KERNEL_MATERN52
    cond = dict(Z=Z, norm_bounds=st.norm_bounds, lengthscale=st.lengthscale, noise=st.noise, kernel=kcode)
    ctx = native.Context(max_n=n, max_d=k, max_q=512)
    grp = native.Context(max_n=n, max_d=k, max_q=512)
    grp.set_option(native.OPT_GROUP_ACQ, 1)
    on_device = k <= 40 and n <= 512                                          # the device optimiser's limits
    group_kernel = group_kernel_possible(n, k)
    assert group_kernel == (name != "n1473")
    bt = native.Batch(1, max_n=n, max_d=k, max_q=512, device_lbfgsb=1 if on_device else 0)
    try:
        for c in (ctx, grp, bt.ctx[0]):
            c.set_option(native.OPT_BESTF_F32, 0)
        ctx.gp_condition(y, **cond)
        grp.gp_condition(y, **cond)
        bt.gp_condition_begin(Z[None], y[None], norm_bounds=st.norm_bounds, lengthscale=st.lengthscale, gp_noise=st.noise,
                              kernel=kcode)
        _, status = bt.gp_wait_eval([X], [float(y.min())], False, native.ACQ_LOG_EI)
        assert not status.any()
        keys, lins = {}, {}
        for tag, c in (("ctx", ctx), ("grp", grp), ("bt", bt.ctx[0])):
            gs = c.gp_state()
            if st.norm_bounds is not None:
                assert np.array_equal(gs["norm_bounds"], st.norm_bounds)
            keys[tag], lins[tag] = A.cached_linear(st, gs)
            assert A.check_conditions(name, st, lins[tag]) == [], (name, tag)      # on the device's own state, not skipped
        lin = lins["ctx"]
        worst, fails = {}, []
        if not group_kernel:               # the same launches on the same state: the comparison below is bit for bit
            assert keys["grp"] == keys["ctx"], "two contexts conditioned alike hold different states"

        def note(path, label, ref, v, g=None):
            rv, rg = A.judge(ref, v, g)
            w = worst.setdefault(path, [0.0, 0.0])
            w[0], w[1] = max(w[0], rv), max(w[1], rg)
            if not (rv <= LIMIT and rg <= LIMIT):
                fails.append((path, label, rv, rg))

        between_worst, between_units = 0.0, 0.0
        for label, acq, mx, best in A.cases(lin):
            ref, gref, bref = (A.cached_scalars(keys[t], label, acq, mx, best) for t in ("ctx", "grp", "bt"))
            out = {}
            for q, path in ((5, "q5"), (6, "q6"), (32, "finish32"), (40, "combine40"), (130, "fast130")):
                out[path] = ctx.acq_eval(X[:q], best, mx, acq)
                note(path, label, ref, *out[path])
            ctx.gp_condition(y, wait=False, **cond)
            out["gemm130"] = (ctx.gp_wait_eval(X, best, mx, acq), None)
            note("gemm130", label, ref, out["gemm130"][0])
            grp.gp_condition(y, wait=False, **cond)
            out["groupgemm130"] = (grp.gp_wait_eval(X, best, mx, acq), None)
            note("groupgemm130", label, gref, out["groupgemm130"][0])
            for q, path in ((5, "group5"), (6, "group6"), (32, "group32"), (40, "group40"), (130, "group130")):
                out[path] = grp.acq_eval(X[:q], best, mx, acq)
                note(path, label, gref, *out[path])
            if not group_kernel:           # the group context on the plain context's launches: the same bits
                for gpath, path in GROUP_TWINS:
                    for a, b in zip(out[gpath], out[path]):
                        if a is not None and not np.array_equal(a, b):
                            fails.append(("the group context beyond k_acq_group differs from the plain one", gpath, label))
            bt.gp_condition_begin(Z[None], y[None], norm_bounds=st.norm_bounds, lengthscale=st.lengthscale,
                                  gp_noise=st.noise, kernel=kcode)
            vb, status = bt.gp_wait_eval([X], [best], mx, acq)
            assert not status.any()
            note("batch130", label, bref, vb[0])
            # pairs of paths on the same queries: (one, other, how many queries)
            pairs = [(out["group32"], out["finish32"], 32), (out["combine40"], out["finish32"], 32),
                     (out["fast130"], out["finish32"], 32), (out["q6"], out["q5"], 5), (out["group6"], out["q5"], 5)]
            if on_device:
                vd, gd = bt.device_acq_eval([X[:32]], [best], mx, acq)
                note("device32", label, bref, vd[0], gd[0])
                pairs.append(((vd[0], gd[0]), out["finish32"], 32))
            deep = label.split(",")[2] in DEEP_MIDDLE
            well = A.well_conditioned(ref)
            between = []
            for (va, ga), (vb_, gb), q in pairs:
                between.append(_verr(va[:q], vb_[:q]))
                rows = np.flatnonzero(well[:q]) if deep else np.arange(q)
                if len(rows):
                    between.append(_rel(ga[:q][rows], gb[:q][rows]))
                if deep:                   # all queries, in the reference's units
                    between_units = max(between_units, A.agreement(ref, ga[:q], gb[:q]))
            between_worst = max(between_worst, max(between))
            if not max(between) < FAMILIES_AGREE:
                fails.append(("families", label, between))
        if not between_units <= FAMILIES_UNITS:
            fails.append(("families, deep middle branch, in units", between_units))
        for tag, c in (("ctx", ctx), ("grp", grp), ("bt", bt.ctx[0])):        # every re-conditioning gave the bits judged
            if (st.name, A.digest(c.gp_state())) != keys[tag]:
                fails.append(("the conditioned state changed between conditionings", tag))
    finally:
        ctx.close()
        grp.close()
        bt.close()
    with capsys.disabled():
        print("\n[log-EI / PI, device / reference units, state %s (n=%d k=%d %s)] " % (name, n, k, st.kernel)
              + "; ".join("%s %.2g/%.2g" % (p, worst[p][0], worst[p][1]) for p in PATHS if p in worst)
              + "; families %.1e, deep middle branch %.2g units; %.1f s" % (between_worst, between_units, time.time() - t0))
    assert not fails, (len(fails), fails[:12])
    assert set(worst) == set(PATHS) - (set() if on_device else {"device32"})
