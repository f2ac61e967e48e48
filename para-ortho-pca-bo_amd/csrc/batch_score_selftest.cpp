// Stand-alone check of what pcabo_batch_acq_score adds to model_state.h: BatchState::value_scorable - the batch has a GP, its
// conditioning has been waited for, no _begin half is open - and the two transitions of the call's halves, which change nothing of the
// model's phase.  Beside it the question of the OTHER scoring (scorable(): it ends a conditioning, or follows a fit) answers as
// before in every state walked through here.  No HIP, no library: g++ batch_score_selftest.cpp (tests/test_batch_score_state_cpu.py
// builds and runs it, plain and with -fsanitize=address,undefined).
#include <cstdio>
#include "model_state.h"

static int failures = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      ++failures;                                            \
      std::fprintf(stderr, "line %d: ", __LINE__);           \
      std::fprintf(stderr, __VA_ARGS__);                     \
      std::fprintf(stderr, "\n");                            \
    }                                                        \
  } while (0)

// what pcabo_batch_acq_score_end hands out for run i (batch_value_score_collect): an active run with a GP of the batch's n
static bool handed_out(const ModelState& r, bool active) { return active && r.conditioned(); }

int main() {
  {
    BatchState b;
    ModelState r[3];
    CHECK(!b.value_scorable() && !b.scorable() && b.gp_ready() == GP_NONE, "a new batch has nothing to score");
    // a conditioning goes out: the other scoring may end it, this one may not look yet
    b.condition_enqueued(40, 6, 4, 0.7, 1e-3, 0);
    for (ModelState& m : r) m.follow(b, m.own().with_k(4).started(0.7, 1e-3));
    CHECK(b.scorable() && !b.value_scorable() && b.gp_ready() == GP_IN_FLIGHT, "in flight: condition_end_eval only");
    b.scoring_begun();
    CHECK(!b.value_scorable() && b.begin_pending(), "its _begin half is open");
    b.scoring_ended();
    for (ModelState& m : r) m.follow(b, m.own().ended(true));
    // waited for, unfitted: condition_end_eval refuses from here on, the values can be had
    CHECK(!b.scorable() && b.value_scorable() && b.gp_ready() == GP_READY && !b.fitted, "conditioned and unfitted: acq_score only");
    const ModelState before = b.m;
    b.value_scoring_begun();
    CHECK(b.value_score_enqueued && b.begin_pending() && !b.value_scorable() && b.gp_ready() == GP_IN_FLIGHT,
          "between the halves every other call on the model waits, a second _begin included");
    CHECK(!b.scorable(), "... and condition_end_eval still has nothing to end");
    CHECK(b.m.n == before.n && b.m.n_base == before.n_base && b.m.have_gp && !b.m.gp_pending, "the model's phase is not touched");
    b.value_scoring_ended();
    CHECK(!b.value_score_enqueued && !b.begin_pending() && b.value_scorable() && !b.scorable(), "as before the call");
    CHECK(b.m.n == before.n && b.m.NP == before.NP && b.m.have_gp && !b.m.gp_pending && b.m.rung == before.rung &&
          b.m.cnt_S == before.cnt_S && b.m.cnt_dirty == before.cnt_dirty, "nothing of the record moved");
    // extended: still scorable by value; a run set aside or parked is not handed out
    b.points_appended(2);
    r[0].follow_extend(b, true, 40);
    r[1].follow_extend(b, false, 40);                     // its pivot failed
    r[2].follow_extend(b, true, 40);
    CHECK(b.extended() && b.value_scorable() && !b.scorable(), "an extended, unfitted batch");
    CHECK(handed_out(r[0], true) && !handed_out(r[1], true) && !handed_out(r[2], false), "live / set aside / parked");
    b.value_scoring_begun();
    b.value_scoring_ended();
    CHECK(r[1].aside_n == 40 && !r[1].conditioned() && r[0].conditioned() && r[0].n == 42, "the members are as the extend left them");
    b.points_taken_back(40);
    for (ModelState& m : r) m.follow_truncate(b, 40);
    CHECK(b.value_scorable() && handed_out(r[1], true), "taken back: every run is live again");
    // the other _begin halves close the door as well
    b.opt_begun(10, 5);
    CHECK(!b.value_scorable(), "an optimiser in flight");
    b.opt_ended();
    b.imap_begun();
    CHECK(!b.value_scorable(), "an inverse map in flight");
    b.imap_ended();
    CHECK(b.value_scorable(), "all halves ended");
    // a fit: both scorings are possible, each with its own half
    b.fit_finished();
    CHECK(b.scorable() && b.value_scorable(), "a fitted batch");
    b.value_scoring_begun();
    CHECK(b.scorable() && !b.value_scorable() && b.begin_pending(), "fitted, a value scoring open (condition_end_eval asks begin_pending's flag)");
    b.value_scoring_ended();
    b.scoring_begun();
    CHECK(!b.value_scorable(), "fitted, the other scoring open");
    b.scoring_ended();
    CHECK(b.scorable() && b.value_scorable() && b.fitted, "both again");
    // a new conditioning starts over
    b.condition_enqueued(41, 6, 4, 0.7, 1e-3, 0);
    CHECK(b.scorable() && !b.value_scorable() && !b.fitted, "in flight again");
  }
  {
    // a conditioning that failed for every run leaves no GP to score
    BatchState b;
    b.condition_enqueued(10, 3, 3, 0.7, 1e-3, 0);
    b.m.condition_failed();
    CHECK(!b.value_scorable() && b.gp_ready() == GP_NONE, "no GP");
  }
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("batch score state: ok\n");
  return 0;
}
