"""UCB on every evaluation path of the device against an extended-precision reference at edge shapes.

The third branch of `acq_scalar_chain` (acq_math.h; kappa in the `best_f` slot) behind every kernel that evaluates the
acquisition - `k_acq_fast<SLAB, NB>`, `k_acq_fused`, `k_acq_group`, `k_acq_combine`, the GEMM scoring and `lb_eval` - is
judged in the error units of `acq_reference.scalars_ucb` (first-order analysis of any fp64 implementation;
`test_ucb_posterior_reference_cpu.py` shows a numpy restatement staying under 4 of each and wrong variants leaving
them).  The limit is 16 in every unit, as in `test_gpu_acq_edges.py`, whose states, queries, paths and entry points
these are; `test_gpu_ucb.py` compares the same paths with a float64 oracle at tolerances measured on the device.

The reference starts from each object's OWN conditioned state (`gp_state()`), read once after conditioning and taken
as exact.  kappa: 0, 0.5, sqrt 2 and 1e3 (the sigma term carries value and gradient), in both directions.

The states are all of `acq_reference.STATES`, the four of the stress region included (n385k65, n449k83, n1025, n1473:
`k_acq_fused<32>` at k > 32, `k_acq_group<2>` past 64 KB of LDS, `k_acq_group<5>` with five live columns, the second
iteration of `grad_partial_sum`'s unrolled loop); at n1473 the group context lies beyond `acq_group_possible` and must
give the plain context's bits (`test_gpu_acq_edges.GROUP_TWINS`).
"""
import time

import numpy as np
import pytest

import acq_reference as A
from test_gpu_acq_edges import FAMILIES_AGREE, GROUP_TWINS, PATHS, _rel, _verr, group_kernel_possible

pytestmark = pytest.mark.gpu

LIMIT = 16.0


@pytest.mark.parametrize("name", list(A.STATES))
def test_ucb_against_the_reference_on_every_path(native, name, capsys):
    """Per state, direction and kappa: every value and every gradient component of the paths of
    `test_gpu_acq_edges.py` within 16 units of the reference on the object's own state; the kernel families agree to
    1e-10; at a clamped variance the kappa term adds nothing to the gradient, bit for bit; kappa = 0 gives the bits of
    +-mean of `gp_posterior`.  Prints the worst ratio per path."""
    t0 = time.time()
    st, _, _ = A.prepared(name)
    n, k, Z, y, X = st.n, st.k, st.Z, st.y, st.X
    kcode = native.KERNEL_RBF if st.kernel == "rbf" else native.KERNEL_MATERN52
    cond = dict(Z=Z, norm_bounds=st.norm_bounds, lengthscale=st.lengthscale, noise=st.noise, kernel=kcode)
    bcond = dict(norm_bounds=st.norm_bounds, lengthscale=st.lengthscale, gp_noise=st.noise, kernel=kcode)
    ctx = native.Context(max_n=n, max_d=k, max_q=512)
    grp = native.Context(max_n=n, max_d=k, max_q=512)
    grp.set_option(native.OPT_GROUP_ACQ, 1)
    on_device = k <= 40 and n <= 512                                          # the device optimiser's limits
    group_kernel = group_kernel_possible(n, k)                                # False at n1473: see GROUP_TWINS
    bt = native.Batch(1, max_n=n, max_d=k, max_q=512, device_lbfgsb=1 if on_device else 0)
    U = native.ACQ_UCB
    try:
        for c in (ctx, grp, bt.ctx[0]):
            c.set_option(native.OPT_BESTF_F32, 0)                             # kappa = sqrt 2 keeps its 64 bits
        ctx.gp_condition(y, **cond)
        grp.gp_condition(y, **cond)
        bt.gp_condition_begin(Z[None], y[None], **bcond)
        _, status = bt.gp_wait_eval([X], [1.0], False, U)
        assert not status.any()
        keys, lins = {}, {}
        for tag, c in (("ctx", ctx), ("grp", grp), ("bt", bt.ctx[0])):
            gs = c.gp_state()
            if st.norm_bounds is not None:
                assert np.array_equal(gs["norm_bounds"], st.norm_bounds)
            keys[tag], lins[tag] = A.cached_linear(st, gs)
            assert A.check_ucb_conditions(name, st, lins[tag]) == [], (name, tag)  # on the device's own state, not skipped
        worst, fails, between_worst = {}, [], 0.0
        if not group_kernel:               # the same launches on the same state: the comparison below is bit for bit
            assert keys["grp"] == keys["ctx"], "two contexts conditioned alike hold different states"
        post_mean = ctx.gp_posterior(X)["mean"]

        def note(path, label, ref, v, g=None):
            rv, rg = A.judge(ref, v, g)
            w = worst.setdefault(path, [0.0, 0.0])
            w[0], w[1] = max(w[0], rv), max(w[1], rg)
            if not (rv <= LIMIT and rg <= LIMIT):
                fails.append((path, label, rv, rg))

        zero = {}                                                              # direction -> path -> gradient at kappa = 0
        for label, acq, mx, kap in A.cases_ucb():
            ref, gref, bref = (A.cached_scalars(keys[t], label, acq, mx, kap) for t in ("ctx", "grp", "bt"))
            out = {}
            for q, path in ((5, "q5"), (6, "q6"), (32, "finish32"), (40, "combine40"), (130, "fast130")):
                out[path] = ctx.acq_eval(X[:q], kap, mx, U)
                note(path, label, ref, *out[path])
            ctx.gp_condition(y, wait=False, **cond)
            gemm = ctx.gp_wait_eval(X, kap, mx, U)
            note("gemm130", label, ref, gemm)
            grp.gp_condition(y, wait=False, **cond)
            groupgemm = grp.gp_wait_eval(X, kap, mx, U)
            note("groupgemm130", label, gref, groupgemm)
            for q, path in ((5, "group5"), (6, "group6"), (32, "group32"), (40, "group40"), (130, "group130")):
                out[path] = grp.acq_eval(X[:q], kap, mx, U)
                note(path, label, gref, *out[path])
            if not group_kernel:           # the group context on the plain context's launches: the same bits
                twins = [(gp, p, a, b) for gp, p in GROUP_TWINS[:5] for a, b in zip(out[gp], out[p])]
                for gpath, path, a, b in twins + [GROUP_TWINS[5] + (groupgemm, gemm)]:
                    if not np.array_equal(a, b):
                        fails.append(("the group context beyond k_acq_group differs from the plain one", gpath, label))
            bt.gp_condition_begin(Z[None], y[None], **bcond)
            vb, status = bt.gp_wait_eval([X], [kap], mx, U)
            assert not status.any()
            note("batch130", label, bref, vb[0])
            pairs = [(out["group32"], out["finish32"], 32), (out["combine40"], out["finish32"], 32),
                     (out["fast130"], out["finish32"], 32), (out["q6"], out["q5"], 5), (out["group6"], out["q5"], 5)]
            if on_device:
                vd, gd = bt.device_acq_eval([X[:32]], [kap], mx, U)
                out["device32"] = (vd[0], gd[0])
                note("device32", label, bref, vd[0], gd[0])
                pairs.append((out["device32"], out["finish32"], 32))
            between = []
            for (va, ga), (vb_, gb), q in pairs:
                between += [_verr(va[:q], vb_[:q]), _rel(ga[:q], gb[:q])]
            between_worst = max(between_worst, max(between))
            if not max(between) < FAMILIES_AGREE:
                fails.append(("families", label, between))
            # exactness.  kappa = 0: fma(0, sigma, +-mean), the scoring's bits of the posterior's mean
            if kap == 0.0:
                zero[mx] = {p: g for p, (_, g) in out.items()}
                v0 = ctx.acq_eval(X, 0.0, mx, U, grad=False)
                if not np.array_equal(v0, post_mean if mx else -post_mean):
                    fails.append(("kappa = 0 is not the posterior's mean, bit for bit", label))
            else:                          # a clamped variance: c_sg = 0, the gradient is that of the mean alone
                for p, (_, g) in out.items():
                    cl = (bref if p == "device32" else gref if p.startswith("group") else ref).clamped[:len(g)]
                    if not np.array_equal(g[cl], zero[mx][p][cl]):
                        fails.append(("the kappa term moves the gradient at a clamped variance", p, label))
        clamped = A.cached_scalars(keys["ctx"], "ucb,0,0", A.UCB, 0, 0.0).clamped[:32]
        if name == "E" and not clamped.all() or name == "mixed" and not (clamped.any() and not clamped.all()):
            fails.append(("the clamped states are not what their names say", int(clamped.sum())))
        for tag, c in (("ctx", ctx), ("grp", grp), ("bt", bt.ctx[0])):        # every re-conditioning gave the bits judged
            if (st.name, A.digest(c.gp_state())) != keys[tag]:
                fails.append(("the conditioned state changed between conditionings", tag))
    finally:
        ctx.close()
        grp.close()
        bt.close()
    with capsys.disabled():
        print("\n[UCB, device / reference units, state %s (n=%d k=%d %s)] " % (name, n, k, st.kernel)
              + "; ".join("%s %.2g/%.2g" % (p, worst[p][0], worst[p][1]) for p in PATHS if p in worst)
              + "; families %.1e; %.1f s" % (between_worst, time.time() - t0))
    assert not fails, (len(fails), fails[:12])
    assert set(worst) == set(PATHS) - (set() if on_device else {"device32"})
