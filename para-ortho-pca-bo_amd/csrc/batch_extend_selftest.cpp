// Stand-alone check of what pcabo_batch_gp_extend / pcabo_batch_gp_truncate add to model_state.h: the batch's n after extend and
// truncate with n_base held, a member set aside and brought back through follow(), the mark cleared by a conditioning, the tickets
// following acq_slabs(NP) across 64 <-> 65.  No HIP, no library: g++ batch_extend_selftest.cpp (tests/test_batch_extend_cpu.py
// builds and runs it, plain and with -fsanitize=address,undefined).  What a member does after its batch's extend and truncate
// (ModelState::follow_extend / follow_truncate), which runs a truncate launches for (RunOwn::rows_beyond) and what a scoring leaves of
// a run set aside (RunOwn::ended) are the functions pcabo_api.hip calls; only the order of the batch's own steps around them is
// restated here (Batch3), as the entry points have it: count, tickets, members.
#include <cstdio>
#include <vector>
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

// The record compares slab counts, it does not compute them (acq_slabs lives with the acquisition kernels).  Any count that differs
// between NP = 64 and NP = 128 serves the checks below; this one is NOT acq_slabs.
static int slabs(int NP) { return NP / PCABO_BS; }

struct Batch3 {
  BatchState b;
  ModelState r[3];
  std::vector<ModelState*> runs{&r[0], &r[1], &r[2]};
  bool active[3] = {true, true, true};
  bool launched[3] = {false, false, false};            // the runs the last truncate had k_ext_truncate work for

  // pcabo_batch_gp_condition_begin + pcabo_batch_gp_condition_end_eval with every factorisation fine
  void condition(int n, int k) {
    b.tickets_reset_if_needed(slabs(round_up(n, PCABO_BS)), runs);
    b.condition_enqueued(n, k, k, 0.7, 1e-3, 0);
    for (ModelState& m : r) m.follow(b, m.own().with_k(k).started(0.7, 1e-3));
    b.scoring_begun();
    b.scoring_ended();
    for (ModelState& m : r) m.follow(b, m.own().ended(true));
  }
  bool takes_part(int i) const { return active[i] && r[i].conditioned(); }
  // pcabo_batch_gp_extend: fails[i] - the pivot of run i failed.  Returns whether the tickets were reset.
  bool extend(int p, const bool* fails) {
    const int n0 = b.m.n;
    bool part[3];
    for (int i = 0; i < 3; ++i) part[i] = takes_part(i);
    b.points_appended(p);
    const bool reset = b.tickets_reset_if_needed(slabs(b.m.NP), runs);
    for (int i = 0; i < 3; ++i) r[i].follow_extend(b, part[i] && !fails[i], n0);
    return reset;
  }
  // pcabo_batch_gp_condition_end_eval on a fitted batch (batch_score_collect with every chol_info 0)
  void score() {
    b.scoring_begun();
    b.scoring_ended();
    for (ModelState& m : r) m.follow(b, m.own().ended(true));
  }
  bool truncate(int n0) {
    CHECK(b.can_truncate_to(n0), "truncate(%d) allowed", n0);
    const int n = b.m.n;
    for (int i = 0; i < 3; ++i) launched[i] = r[i].own().rows_beyond(n0, n);
    b.points_taken_back(n0);
    const bool reset = b.tickets_reset_if_needed(slabs(b.m.NP), runs);
    for (ModelState& m : r) m.follow_truncate(b, n0);
    return reset;
  }
};

int main() {
  const bool none[3] = {false, false, false}, second[3] = {false, true, false};
  {
    Batch3 t;
    t.condition(64, 5);
    CHECK(t.b.gp_ready() == GP_READY && !t.b.extended(), "conditioned, nothing appended");
    CHECK(t.b.m.n == 64 && t.b.m.n_base == 64 && t.b.m.NP == 64 && t.b.m.cnt_S == slabs(64), "64 points, one block");
    for (ModelState& m : t.r) m.rt_rebuilt();
    // 64 -> 65: NP grows, the tickets follow, n_base is held, the members' root inverse is outdated
    CHECK(t.extend(1, none), "64 -> 65 changes acq_slabs: the tickets are reset");
    CHECK(t.b.m.n == 65 && t.b.m.n_base == 64 && t.b.m.NP == 128 && t.b.extended(), "65 points of which 64 are the base");
    CHECK(t.b.m.cnt_S == slabs(128) && !t.b.m.cnt_dirty, "the tickets are those of NP = 128");
    for (ModelState& m : t.r)
      CHECK(m.n == 65 && m.n_base == 64 && m.NP == 128 && m.conditioned() && m.rt_stale && m.cnt_S == slabs(128) && m.aside_n < 0,
            "a member follows: n %d n_base %d NP %d", m.n, m.n_base, m.NP);
    CHECK(!t.extend(2, none), "65 -> 67 keeps NP: no reset");
    CHECK(t.b.m.n == 67 && t.b.m.n_base == 64, "67 points");
    CHECK(!t.b.can_truncate_to(63) && !t.b.can_truncate_to(68) && t.b.can_truncate_to(64) && t.b.can_truncate_to(67), "n_base .. n");
    CHECK(!t.truncate(65), "67 -> 65 keeps NP");
    CHECK(t.truncate(64), "65 -> 64 changes acq_slabs back: the tickets are reset");
    CHECK(t.b.m.n == 64 && t.b.m.NP == 64 && t.b.m.cnt_S == slabs(64) && !t.b.extended(), "back at the base");
    for (ModelState& m : t.r) CHECK(m.n == 64 && m.NP == 64 && m.conditioned() && m.cnt_S == slabs(64), "the members are back");
  }
  {
    // a pivot that fails in run 1: set aside at the n of entry, skipped, brought back only by a truncate that reaches that n
    Batch3 t;
    t.condition(63, 5);
    t.extend(1, none);                                   // 64 points everywhere
    const double rung1 = t.r[1].rung;
    t.extend(3, second);                                 // run 1 fails: valid up to 64
    CHECK(t.b.m.n == 67 && t.r[1].n == 67, "the batch goes on, the member's counts are the batch's");
    CHECK(!t.r[1].conditioned() && t.r[1].aside_n == 64 && t.r[1].own().is_aside(), "run 1 is set aside at 64");
    CHECK(t.r[0].conditioned() && t.r[2].conditioned() && t.r[0].aside_n < 0, "the others are live");
    CHECK(!t.takes_part(1) && t.takes_part(0), "a run set aside takes no part");
    t.extend(1, none);                                   // a further extend: run 1 stays where it is
    CHECK(t.r[1].aside_n == 64 && !t.r[1].conditioned() && t.b.m.n == 68, "still aside at 64");
    // a scoring of the extended batch (after a fit the batch stays scorable) ends well for every run: run 1 stays aside
    t.b.fit_finished();
    CHECK(t.b.scorable() && t.b.extended(), "a fitted, extended batch can be scored");
    t.score();
    CHECK(!t.r[1].conditioned() && t.r[1].aside_n == 64 && !t.takes_part(1), "a scoring does not bring a run set aside back");
    CHECK(t.r[1].holds_factors() && t.r[1].rows_held() == 64 && t.r[0].rows_held() == 68, "its factors can be read, at 64 rows");
    CHECK(t.r[0].conditioned() && t.r[2].conditioned(), "the live runs stay live");
    for (ModelState& m : t.r) m.rt_rebuilt();
    t.truncate(67);
    CHECK(t.launched[0] && !t.launched[1] && t.launched[2], "68 -> 67: the live runs only");
    CHECK(t.r[0].rt_stale && !t.r[1].rt_stale, "whose factors changed");
    CHECK(!t.r[1].conditioned() && t.r[1].aside_n == 64, "67 is beyond what run 1 holds: still aside");
    CHECK(!t.r[1].own().revives_at(65) && t.r[1].own().revives_at(64) && t.r[1].own().revives_at(63), "what brings it back");
    t.truncate(64);
    CHECK(t.launched[0] && !t.launched[1], "67 -> 64: run 1 holds exactly 64 rows, nothing is launched for it");
    CHECK(!t.r[1].rt_stale, "... and its transposed root inverse stays as it was");
    CHECK(t.r[1].conditioned() && t.r[1].aside_n < 0 && t.r[1].n == 64 && t.r[1].rung == rung1, "live again at 64, its rung kept");
    t.extend(2, second);                                 // fails again at entry 64, then all the way back
    CHECK(t.r[1].aside_n == 64, "aside at 64 again");
    t.truncate(63);
    CHECK(t.launched[0] && t.launched[1] && t.launched[2], "66 -> 63: run 1 holds 64 rows, one of them is taken back");
    CHECK(t.r[1].rt_stale, "... its factors changed");
    CHECK(t.r[1].conditioned() && t.r[1].n == 63 && t.b.m.n == t.b.m.n_base, "n_base brings every run back");
    t.truncate(63);
    CHECK(!t.launched[0] && !t.launched[1] && !t.launched[2], "n0 == n: nothing to do");
  }
  {
    // a parked run with a GP is out of step as well; a run without a GP has nothing to set aside; a conditioning clears the mark
    Batch3 t;
    t.condition(20, 3);
    t.active[2] = false;
    t.r[0].follow(t.b, t.r[0].own().ended(false));       // run 0: its factorisation failed
    t.extend(2, none);
    CHECK(!t.r[0].conditioned() && t.r[0].aside_n < 0, "no GP: nothing set aside");
    CHECK(!t.r[2].conditioned() && t.r[2].aside_n == 20, "the parked run is at n_base, out of step");
    CHECK(t.r[1].conditioned() && t.r[1].n == 22, "the one live run took the points");
    t.truncate(20);
    CHECK(!t.r[0].conditioned() && t.r[2].conditioned() && t.r[2].aside_n < 0, "the truncate brings back what had a GP, nothing else");
    t.extend(1, second);
    CHECK(t.r[1].aside_n == 20 && t.r[2].aside_n == 20, "both aside");
    t.condition(30, 3);
    for (ModelState& m : t.r) CHECK(m.conditioned() && m.aside_n < 0 && m.n == 30 && m.n_base == 30, "a conditioning starts over");
    CHECK(!t.b.extended(), "nothing appended after a conditioning");
    // a fit or likelihood evaluation forgets the extension before its first round
    t.extend(40, none);
    CHECK(t.b.m.n == 70 && t.b.m.NP == 128, "70 points");
    t.b.extension_forgotten();
    CHECK(t.b.m.n == 30 && t.b.m.NP == 64 && t.b.tickets_need_reset(slabs(64), t.runs), "back at 30, the tickets are those of 128");
  }
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("batch extend state: ok\n");
  return 0;
}
