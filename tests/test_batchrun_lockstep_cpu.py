"""The lock-step iteration of pcabo/batchrun.py, pinned on the CPU: whole batches of BatchedPCABO and BatchedVanillaBO over a
scripted stand-in for `_native.Batch` (tests/lockstep_fake.py), every case held to the digests that the batchrun.py of the
commit named in tests/golden/batch_lockstep_digests.json gave - trajectories, counters, trace entries, generator end states,
warnings, yield labels and the batch's whole call log.  The GPU tests compare whole runs of whichever class they use; the rare
paths (retry, every cause of parking, a wrong guess of k, the PI pick, the trace in device mode) are forced here, for both."""
import json

import pytest

import lockstep_fake as LF

CASES = LF.cases()
_done = {}


@pytest.fixture(scope="module")
def golden():
    with open(LF.GOLDEN) as f:
        return json.load(f)


def _both_drives(cid, native, monkeypatch):
    if cid not in _done:
        monkeypatch.setattr(native, "Batch", LF.FakeBatch)
        _done[cid] = (LF.run_case(CASES[cid], "iteration"), LF.run_case(CASES[cid], "interleaved"))
    return _done[cid]


def _first_difference(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return "call %d: got %r, recorded %r" % (i, a, b)
    return "%d calls, recorded %d" % (len(got), len(want))


def test_the_golden_file_holds_exactly_the_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES) and golden["recorded_from"] == LF.RECORDED_FROM
    assert sorted(golden["call_logs"]) == sorted(LF.FULL_LOGS)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_lockstep_batch_takes_the_recorded_path(native, monkeypatch, golden, cid):
    (by_iteration, log), (interleaved, log_interleaved) = _both_drives(cid, native, monkeypatch)
    want = golden["cases"][cid]
    if cid in golden["call_logs"]:
        assert log == golden["call_logs"][cid], _first_difference(log, golden["call_logs"][cid])
    assert log_interleaved == log, _first_difference(log_interleaved, log)
    assert interleaved == by_iteration, {k: (by_iteration[k], interleaved[k]) for k in want if by_iteration[k] != interleaved[k]}
    assert by_iteration == want, {k: (by_iteration.get(k), want[k]) for k in want if by_iteration.get(k) != want[k]}


@pytest.mark.parametrize("cls", ["pca", "vanilla"])
def test_the_scripts_reach_every_rare_path(native, monkeypatch, cls):
    fired, statuses = set(), set()
    for cid in sorted(CASES):
        if cid.startswith(cls + "-"):
            (got, _), _ = _both_drives(cid, native, monkeypatch)
            fired.update(e.split("/")[0] for e in got["fired"])
            statuses.update(v for (e, _, _), v in CASES[cid][2].items() if e == "opt_status")
            assert len(got["fired"]) - sum(e.startswith("k_changed") for e in got["fired"]) == len(CASES[cid][2]), got["fired"]
    assert fired >= set(LF.EVENTS) and statuses == {-4, -7}
    if cls == "pca":
        assert "k_changed" in fired            # (the engine built with last iteration's k was the wrong one)
