"""q candidates per iteration in the lock-step loop of pcabo/batchrun.py (_later_proposals), on the CPU: whole batches over the
scripted stand-in of tests/lockstep_fake.py, grown by the calls the later proposals make (gp_posterior, gp_extend, gp_truncate,
acq_score_begin / _end).  With q = 3, four runs, n_DoE 10 and budget 26 (10 -> 13 -> ... -> 25 -> 26): the runs stay in step, what is
drawn ahead is drawn for n + q_eff points, an extend that fails parks its run alone, botorch's retry of a later proposal goes
through the member context while the batch is extended, the interleaved drive makes the calls of the straight one - and with q = 1
spelled out the loop is the recorded one (tests/golden/batch_lockstep_digests.json)."""
import json
import warnings

import numpy as np
import pytest

import lockstep_fake as LF

Q = 3


class QFakeBatch(LF.FakeBatch):
    """FakeBatch with the model calls of the later proposals.  `n` stays the n of the conditioning (the script's key); `held` is
    what the models hold.  Script keys of four entries - (event, run, n, proposal) - fire at that proposal (1, 2, ...) only."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.held, self.proposal, self.aside = 0, 0, set()

    def _event(self, event, b):
        if self.proposal:
            v = self.script.pop((event, b, self.n, self.proposal), None)
            if v is not None:
                self.fired.append(("%s@%d" % (event, self.proposal), b, self.n))      # (three entries: run_case formats them)
            return v
        return super()._event(event, b)

    def wpca_gp_condition_begin(self, X, *a, **kw):
        super().wpca_gp_condition_begin(X, *a, **kw)
        self.held, self.proposal, self.aside = self.n, 0, set()

    def gp_condition_begin(self, Z, *a, **kw):
        super().gp_condition_begin(Z, *a, **kw)
        self.held, self.proposal, self.aside = self.n, 0, set()

    @property
    def n_base(self):
        return self.n

    def gp_posterior(self, Xq_list, observation_noise=False, covariance=False):
        assert not observation_noise and not covariance
        self._log("gp_posterior", self.held, " ".join(LF._h(x) for x in Xq_list))
        return [{"mean": 40.0 + 10.0 * LF._value(x) - 0.5 * self.held, "variance": np.ones(len(x))} if self.active[b] else None
                for b, x in enumerate(Xq_list)]

    def gp_extend(self, Zp_list, y=None):
        self.proposal += 1
        self._log("gp_extend", self.held, " ".join(LF._h(z) for z in Zp_list), LF._h(y))
        status = np.zeros(self.B, dtype=np.int32)
        for b in range(self.B):
            if not self.active[b] or b in self.aside:
                status[b] = -1
            elif self._event("extend_status", b):
                status[b] = -2
                self.aside.add(b)
        self.held += 1
        return self.held, status

    def gp_truncate(self, n0=None):
        n0 = self.n if n0 is None else n0
        self._log("gp_truncate", self.held, n0)
        assert self.n <= n0 <= self.held
        self.held, self.proposal, self.aside = n0, 0, set()
        return n0

    def set_active(self, active):
        assert self.held == self.n, "the library refuses a change of the flags while points are appended"
        super().set_active(active)

    def acq_score_begin(self, Xq_list, best_f, maximize=False, acq=0):
        assert self.held > self.n
        self._log("acq_score_begin", self.held, " ".join(LF._h(x) for x in Xq_list), LF._h(np.asarray(best_f, dtype=np.float64)),
                  int(bool(maximize)), int(acq), "in_row_buffer=%d" % all(x.base is self._raw_buf for x in Xq_list))
        return ([np.array(x, dtype=np.float64) for x in Xq_list], int(acq))

    def acq_score_end(self, token):
        raw, acq = token
        vals = np.stack([self._values(x, acq) + 0.001 * self.held for x in raw])
        status = np.array([-1 if (not self.active[b] or b in self.aside) else 0 for b in range(self.B)], dtype=np.int32)
        self._log("acq_score_end", LF._h(vals), LF._h(status))
        return vals, status

    def _optimise(self, ics_list, bounds_list, acq, batch_limit):
        outs, status = super()._optimise(ics_list, bounds_list, acq, batch_limit)
        for b in self.aside:                      # (the library skips a run set aside)
            status[b] = -1
        return outs, status


def _runner(native, monkeypatch, cls="pca", script=None, **kw):
    from pcabo import batchrun
    from pcabo.bbob import BBOBProblem
    monkeypatch.setattr(native, "Batch", QFakeBatch)
    LF.FakeBatch.script, LF.FakeBatch.created = dict(script or {}), []
    return (batchrun.BatchedPCABO if cls == "pca" else batchrun.BatchedVanillaBO)(
        [BBOBProblem(LF.FID, i, LF.DIM) for i in range(LF.B)], [1000 * LF.FID + 10 * LF.DIM + i for i in range(LF.B)],
        LF.BUDGET, LF.N_DOE, **kw)


@pytest.mark.parametrize("cls", ["pca", "vanilla"])
@pytest.mark.parametrize("kern", ["group", "device"])
def test_runs_stay_in_step_and_what_is_drawn_ahead_fits(native, monkeypatch, cls, kern):
    r = _runner(native, monkeypatch, cls, q=Q, acq_kernel=kern)
    seen = []
    try:
        r.start()
        (bt,) = LF.FakeBatch.created
        while r.n < r.budget:
            n = r.n
            q_eff = min(Q, r.budget - n)
            r.iteration()
            assert {len(f) for f in r.f_evals} == {n + q_eff} == {len(x) for x in r.x_evals}
            assert bt.held == bt.n == n                                  # taken back
            if cls == "pca" and n + q_eff < r.budget:
                assert r._noise_next.shape == (LF.B, n + q_eff, LF.DIM)
                assert all(r._noise_ahead[b].result().shape == (n + q_eff, LF.DIM) for b in range(LF.B))
            else:
                assert not r._noise_ahead
            assert (len(r._engines_ahead) == LF.B) == (n + q_eff < r.budget)
            seen.append((n, q_eff))
    finally:
        r.finish()
    assert seen == [(10, 3), (13, 3), (16, 3), (19, 3), (22, 3), (25, 1)]
    assert len(r.lbfgsb_info) == 16 and all(f is None for f in r.failed)
    names = [line.split()[0] for line in bt.log]
    per_iteration = ["gp_posterior", "gp_extend", "acq_score_begin", "acq_score_end"]
    assert [nm for nm in names if nm in per_iteration + ["gp_truncate"]] == (per_iteration * 2 + ["gp_truncate"]) * 5
    assert names.count("gp_eval_begin") == 6 and names.count("inverse_map_begin") == (16 if cls == "pca" else 0)
    opt = "optimize_begin" if kern == "device" else "optimize_acqf"
    assert names.count(opt) == 16
    # every later proposal is scored and optimised with the scalar moved by what the one before it is believed to be worth
    held = [int(line.split()[1]) for line in bt.log if line.startswith("acq_score_begin")]
    assert held == [n + j for n in (10, 13, 16, 19, 22) for j in (1, 2)]
    assert all("in_row_buffer=1" in line for line in bt.log if line.startswith("acq_score_begin"))


@pytest.mark.parametrize("strategy", ["kriging_believer", "constant_liar_min", "constant_liar_mean", "constant_liar_max"])
def test_the_scalars_of_the_later_proposals(native, monkeypatch, strategy):
    r = _runner(native, monkeypatch, "pca", q=Q, q_strategy=strategy, record_trace=True)
    r.run()
    (bt,) = LF.FakeBatch.created
    assert ("gp_posterior" in " ".join(bt.log)) == (strategy == "kriging_believer")
    pick = {"constant_liar_min": min, "constant_liar_mean": lambda f: float(np.mean(np.asarray(f, dtype=np.float64))),
            "constant_liar_max": max}.get(strategy)
    assert len(r.trace) == 6 * LF.B
    for t in r.trace:
        s = t["best_f"]
        assert len(t.get("proposals", [])) == (2 if t["n"] < 25 else 0)
        for p in t.get("proposals", []):
            if pick is not None:
                assert p["believed"] == pick(r.f_evals[t["b"]][: t["n"]])
            assert p["best_f"] == min(s, p["believed"])
            assert p["chosen"] == int(np.argmax(p["vals"]))
            s = p["best_f"]


def test_an_extend_that_fails_parks_its_run_alone(native, monkeypatch):
    r = _runner(native, monkeypatch, "pca", script={("extend_status", 2, 13, 2): True}, q=Q)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        r.run()
    (bt,) = LF.FakeBatch.created
    assert [e for e in bt.fired if e[0] != "k_changed"] == [("extend_status@2", 2, 13)]
    assert r.failed[2] is not None and r.failed[2][0] == 13 and "proposal 1" in r.failed[2][1]
    assert [f is None for f in r.failed] == [True, True, False, True]
    assert len(r.f_evals[2]) == 13 and all(len(r.f_evals[b]) == LF.BUDGET for b in (0, 1, 3))
    assert any("run 2" in str(w.message) and "proposal 1" in str(w.message) for w in caught)
    # the flag reaches the library once the points are taken back (QFakeBatch.set_active asserts it), and only once
    names = [line.split()[0] for line in bt.log]
    i = names.index("set_active")
    assert names[i - 1] == "gp_truncate" and bt.log[i] == "set_active 1101" and names.count("set_active") == 1


def test_a_retry_of_a_later_proposal_goes_through_the_member(native, monkeypatch):
    r = _runner(native, monkeypatch, "pca", script={("failed", 1, 16, 1): True}, q=Q)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        r.run()
    (bt,) = LF.FakeBatch.created
    assert [e for e in bt.fired if e[0] != "k_changed"] == [("failed@1", 1, 16)] and r.retries == 1 and all(f is None for f in r.failed)
    assert any("trying again" in str(w.message) for w in caught)
    names = [line.split()[0] for line in bt.log]
    i = names.index("ctx1.acq_eval")
    assert names[i + 1] == "ctx1.optimize_acqf"
    before = names[:i]
    last_extend = len(before) - 1 - before[::-1].index("gp_extend")
    assert "gp_truncate" not in names[last_extend:i]                     # the batch is still extended: the member's model is M_1
    assert bt.log[last_extend].split()[1] == "16"                        # the first extend of the iteration at n = 16
    assert all(len(f) == LF.BUDGET for f in r.f_evals)


@pytest.mark.parametrize("cls,kern", [("pca", "group"), ("pca", "device"), ("vanilla", "device")])
def test_interleaved_is_straight_through(native, monkeypatch, cls, kern):
    monkeypatch.setattr(native, "Batch", QFakeBatch)
    script = {("extend_status", 0, 19, 1): True, ("failed", 3, 13, 2): True, ("failed", 2, 16): True}
    case = (cls, dict(acq_kernel=kern, q=Q, record_trace=True), script)
    straight, log = LF.run_case(case, "iteration")
    interleaved, log_interleaved = LF.run_case(case, "interleaved")
    assert log_interleaved == log and interleaved == straight
    assert len(straight["fired"]) >= 3


@pytest.mark.parametrize("cid", ["pca-group-EI-nofit-off", "pca-device-EI-nofit-on", "vanilla-group-PI-fit-filter",
                                 "vanilla-device-UCB-nofit-off", "pca-group-EI-nofit-on-max"])
def test_q1_spelled_out_is_the_recorded_loop(native, monkeypatch, cid):
    monkeypatch.setattr(native, "Batch", QFakeBatch)
    with open(LF.GOLDEN) as f:
        golden = json.load(f)
    cls, kw, script = LF.cases()[cid]
    got, log = LF.run_case((cls, dict(kw, q=1, q_strategy="kriging_believer"), script), "iteration")
    want = golden["cases"][cid]
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
    if cid in golden["call_logs"]:
        assert log == golden["call_logs"][cid]
