// Where a model stands between the calls of the C ABI: ONE record (ModelState) for a context and, once, for the runs of a batch
// together (BatchState: the record plus the batch's pending _begin halves).  No HIP: plain arithmetic and flags, included by
// pcabo_api.hip and checked on the CPU by host_selftest.cpp (test_model_state), plain and under the sanitizer builds.
//
// pcabo_api.hip reads the fields and changes them ONLY through the transitions below, each named after what happened; the
// preconditions its entry points check are the const questions.  The record answers; the entry points word the refusals.
// A member run of a batch gets its record from the batch's by follow() and nothing else.  DESIGN.md section 3.1 has the table.
#pragma once
#include "ctx_layout.h"

enum GpReady { GP_READY, GP_IN_FLIGHT, GP_NONE };      // can a call on the conditioned model go ahead?

struct BatchState;
// what a member run of a batch has of its own: its reduced dimension, how its factorisation ended, and - after a lock-step fit -
// the hyperparameters it was conditioned at (before a fit: the batch's shared ones)
// aside_n >= 0: the run is SET ASIDE - it holds a GP of aside_n points while its batch has appended more (pcabo_batch_gp_extend: its
// pivot failed, or it did not take part).  It counts as a run without a GP until the batch is truncated to n0 <= aside_n.
struct RunOwn {
  int k; double rung; bool have_gp; double lengthscale, noise; int aside_n = -1;
  RunOwn with_k(int k_) const { return {k_, rung, have_gp, lengthscale, noise, aside_n}; }          // its wPCA was collected
  RunOwn started(double ls, double s2) const { return {k, 0.0, false, ls, s2, -1}; }                // a conditioning of it went out
  // ... and ended.  A run set aside had no conditioning: a scoring of its extended, fitted batch ends without a word on it
  RunOwn ended(bool ok) const { return is_aside() ? *this : RunOwn{k, rung, ok, lengthscale, noise, -1}; }
  bool is_aside() const { return aside_n >= 0; }
  bool revives_at(int n0) const { return is_aside() && n0 <= aside_n; }                             // would a truncate to n0 bring it back?
  // does a truncate of its batch from n to n0 have rows of this run to take back?  A live run holds n, one that the truncate brings
  // back holds aside_n; a run that stays aside, or has no GP, is left alone
  bool rows_beyond(int n0, int n) const { return have_gp ? n > n0 : revives_at(n0) && aside_n > n0; }
  // the batch went on from n_valid points without it: a run with a GP is set aside, one set aside already keeps its smaller n
  RunOwn set_aside(int n_valid) const {
    if (!have_gp && !is_aside()) return *this;                                                      // (no GP: nothing to keep)
    return {k, rung, false, lengthscale, noise, is_aside() && aside_n < n_valid ? aside_n : n_valid};
  }
  RunOwn truncated(int n0) const { return revives_at(n0) ? RunOwn{k, rung, true, lengthscale, noise, -1} : *this; }
};

struct ModelState {
  // shape: n points (n_base of them from the last conditioning or fit, the others appended by pcabo_gp_extend), d inputs, k reduced
  // dimensions, KP = round_up(k, 4), NP = round_up(n, PCABO_BS)
  int n = 0, n_base = 0, d = 0, k = 0, KP = 0, NP = 0;
  // hyperparameters as conditioned; rung: the jitter the factorisation ended on (0, 1e-8, 1e-7, 1e-6), part of K's diagonal as factored
  double lengthscale = 0.0, noise = 0.0; int kernel = 0; double rung = 0.0;
  // phases.  wpca_uncollected: a wPCA (of wpca_n x wpca_d) whose results have not been waited for; zn_recorded: the event behind
  // k_znorm belongs to the conditioning in flight; rt_stale: the transposed root inverse the device optimiser reads is outdated
  bool have_wpca = false, wpca_uncollected = false; int wpca_n = 0, wpca_d = 0;
  bool gp_pending = false, have_gp = false, zn_recorded = false, rt_stale = false;
  // per-query tickets: the slab-group count they are consistent with / a launch may have died half-way
  int cnt_S = 0; bool cnt_dirty = true;
  // eigenvector ping-pong: the buffer the last Jacobi wrote, and the d it was for (the next one of the same d starts from it)
  int gcur = 0, vprev_d = 0;
  // a member run of a batch only: set aside with a GP of aside_n points (RunOwn), -1: in step with its batch
  int aside_n = -1;

  // ---- questions ----
  bool in_flight() const { return gp_pending; }
  bool conditioned() const { return have_gp; }
  GpReady gp_ready() const { return gp_pending ? GP_IN_FLIGHT : have_gp ? GP_READY : GP_NONE; }
  bool wpca_known() const { return wpca_uncollected || have_wpca; }
  bool wpca_matches(int n_, int k_) const { return have_wpca && n == n_ && k == k_; }      // may a conditioning pass Z == NULL?
  bool warm_start(int d_) const { return vprev_d == d_; }
  bool tickets_need_reset(int slabs) const { return slabs != cnt_S || cnt_dirty; }
  RunOwn own() const { return {k, rung, have_gp, lengthscale, noise, aside_n}; }

  // ---- transitions ----
  void wpca_enqueued(int n_, int d_) { gcur ^= 1; vprev_d = d_; wpca_n = n_; wpca_d = d_; }
  void points_replaced(int n_) { n = n_; have_gp = false; }          // a wPCA on its own: the GP, if any, was of other points
  void wpca_collected(int k_) { d = wpca_d; k = k_; KP = round_up(k_, 4); have_wpca = true; wpca_uncollected = false; }
  // k_ < 0: the reduced dimension is still on the device, the wPCA in flight will say
  void condition_enqueued(int n_, int k_, double lengthscale_, double noise_, int kernel_, bool zn) {
    n = n_base = n_; NP = round_up(n_, PCABO_BS); rung = 0.0;
    if (k_ >= 0) { k = k_; KP = round_up(k_, 4); } else wpca_uncollected = true;
    lengthscale = lengthscale_; noise = noise_; kernel = kernel_;
    have_gp = false; gp_pending = true; zn_recorded = zn;
  }
  bool zn_consumed() { const bool z = zn_recorded; zn_recorded = false; return z; }
  void condition_ended_ok(double rung_) { gp_pending = false; have_gp = true; rung = rung_; }
  void condition_failed() { gp_pending = false; have_gp = false; }
  void n_changed(int n_) { n = n_; NP = round_up(n_, PCABO_BS); rt_stale = true; }      // extend / truncate: n_base is held
  void gram_fetched() { rt_stale = true; }                           // K was built where the transposed root inverse lay
  void rt_wanted() { if (have_gp) rt_stale = true; }                 // the device optimiser was switched on behind a conditioning
  void rt_rebuilt() { rt_stale = false; }
  void root_changed() { rt_stale = true; }                           // a member's L and R grew or shrank with its batch's
  void launch_may_have_died() { cnt_dirty = true; }
  void tickets_reset(int slabs) { cnt_S = slabs; cnt_dirty = false; }
  // question and transition in one: true = the caller enqueues the memset of the tickets now
  bool tickets_reset_if_needed(int slabs) { const bool need = tickets_need_reset(slabs); if (need) tickets_reset(slabs); return need; }
  inline void follow(const BatchState& b, const RunOwn& o);          // a member run after any transition of its batch
  // a member after its batch's extend (took: it took the points; otherwise it is set aside at n_entry, the batch's n before the
  // call) and after its batch's truncate to n0 - the ONE statement of these two steps, for pcabo_api.hip and the record's checks
  inline void follow_extend(const BatchState& b, bool took, int n_entry);
  inline void follow_truncate(const BatchState& b, int n0);
  // a member set aside still holds a model: its factors can be READ (pcabo_get_gp_state, which launches nothing), at rows_held()
  bool holds_factors() const { return have_gp || aside_n >= 0; }
  int rows_held() const { return aside_n >= 0 ? aside_n : n; }
};

struct BatchState {
  ModelState m;                          // of all runs together (they advance in lock-step); k, KP and rung are each run's own
  bool fitted = false;                   // the runs carry their own hyperparameters (a lock-step fit has finished)
  bool score_enqueued = false;           // pcabo_batch_gp_condition_end_eval_begin without its _end yet
  bool imap_enqueued = false;            // pcabo_batch_inverse_map_begin without its _end yet
  bool opt_enqueued = false; int opt_restarts = 0, opt_limit = 0;      // pcabo_batch_optimize_acqf_begin without its _end yet
  bool value_score_enqueued = false;     // pcabo_batch_acq_score_begin without its _end yet

  // ---- questions ----
  bool begin_pending() const { return score_enqueued || opt_enqueued || imap_enqueued || value_score_enqueued; }
  GpReady gp_ready() const { return m.gp_pending || begin_pending() ? GP_IN_FLIGHT : m.have_gp ? GP_READY : GP_NONE; }
  bool scorable() const { return m.gp_pending || fitted; }           // a conditioning in flight, or a fit (waited for already)
  // pcabo_batch_acq_score: values on the model as it stands - the batch has a GP, its conditioning has been waited for and no
  // _begin half is open; fitted or not, extended or not.  (scorable() above is the other scoring's question: it ENDS a conditioning.)
  bool value_scorable() const { return gp_ready() == GP_READY; }
  bool anything_enqueued() const { return m.wpca_uncollected || m.n != 0; }
  bool wpca_on_host() const { return m.n != 0 && !m.wpca_uncollected; }
  bool extended() const { return m.n > m.n_base; }                   // points appended by pcabo_batch_gp_extend and not taken back
  bool can_truncate_to(int n0) const { return n0 >= m.n_base && n0 <= m.n; }
  bool opt_matches(int restarts, int limit) const { return opt_enqueued && opt_restarts == restarts && opt_limit == limit; }
  // a reset is due when the batch's record OR any member's says so (set_err marks the member a single-context call ran on)
  template <class Runs> bool tickets_need_reset(int slabs, const Runs& runs) const {
    bool need = m.tickets_need_reset(slabs);
    for (const ModelState* r : runs) need = need || r->cnt_dirty;
    return need;
  }

  // ---- transitions ----
  void condition_enqueued(int n_, int d_, int k_, double lengthscale_, double noise_, int kernel_) {
    m.condition_enqueued(n_, k_, lengthscale_, noise_, kernel_, false);
    if (k_ >= 0) m.wpca_uncollected = false;           // no wPCA goes with this conditioning
    m.d = d_; m.have_wpca = false; fitted = false;
  }
  void wpca_collected() { m.have_wpca = true; m.wpca_uncollected = false; }
  // pcabo_batch_gp_extend / pcabo_batch_gp_truncate: all runs share the new n, n_base is held (the members: follow + root_changed)
  void points_appended(int p) { m.n += p; m.NP = round_up(m.n, PCABO_BS); }
  void points_taken_back(int n0) { m.n = n0; m.NP = round_up(n0, PCABO_BS); }
  void extension_forgotten() { points_taken_back(m.n_base); }        // a fit or likelihood evaluation starts over from n_base
  void fit_finished() { m.gp_pending = false; m.have_gp = true; fitted = true; }
  void scoring_begun() { score_enqueued = true; }
  void scoring_ended() { score_enqueued = false; m.gp_pending = false; m.have_gp = true; }
  void value_scoring_begun() { value_score_enqueued = true; }          // the model's phase is not touched: nothing ends, nothing starts
  void value_scoring_ended() { value_score_enqueued = false; }
  void imap_begun() { imap_enqueued = true; }
  void imap_ended() { imap_enqueued = false; }
  void opt_begun(int restarts, int limit) { opt_enqueued = true; opt_restarts = restarts; opt_limit = limit; }
  void opt_ended() { opt_enqueued = false; }
  template <class Runs> void tickets_reset(int slabs, const Runs& runs) {
    m.tickets_reset(slabs);
    for (ModelState* r : runs) r->tickets_reset(slabs);
  }
  template <class Runs> bool tickets_reset_if_needed(int slabs, const Runs& runs) {
    const bool need = tickets_need_reset(slabs, runs);
    if (need) tickets_reset(slabs, runs);
    return need;
  }
};

// The ONE way a member's record is written by its batch.  From the batch: the shape but k, the kernel, the wPCA's phase, the
// ping-pong and the ticket count.  The run's own: RunOwn (with its set-aside mark).  A member never has a conditioning or a wPCA of its own in
// flight.  Kept: what only calls on the member itself change (rt_stale, zn_recorded, wpca_n / wpca_d) and its dirty mark, which only a reset clears.
inline void ModelState::follow(const BatchState& b, const RunOwn& o) {
  n = b.m.n; n_base = b.m.n_base; d = b.m.d; NP = b.m.NP; kernel = b.m.kernel;
  have_wpca = b.m.have_wpca; gcur = b.m.gcur; vprev_d = b.m.vprev_d;
  cnt_S = b.m.cnt_S; cnt_dirty = cnt_dirty || b.m.cnt_dirty;
  k = o.k; KP = round_up(o.k, 4); rung = o.rung; have_gp = o.have_gp; lengthscale = o.lengthscale; noise = o.noise;
  aside_n = o.aside_n;
  gp_pending = false; wpca_uncollected = false;
}
inline void ModelState::follow_extend(const BatchState& b, bool took, int n_entry) {
  follow(b, took ? own() : own().set_aside(n_entry));
  if (took) root_changed();
}
inline void ModelState::follow_truncate(const BatchState& b, int n0) {
  const bool taken_back = own().rows_beyond(n0, n);                  // (n: still the batch's before the call)
  follow(b, own().truncated(n0));
  if (taken_back) root_changed();
}
