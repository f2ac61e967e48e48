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
struct RunOwn {
  int k; double rung; bool have_gp; double lengthscale, noise;
  RunOwn with_k(int k_) const { return {k_, rung, have_gp, lengthscale, noise}; }                   // its wPCA was collected
  RunOwn started(double ls, double s2) const { return {k, 0.0, false, ls, s2}; }                    // a conditioning of it went out
  RunOwn ended(bool ok) const { return {k, rung, ok, lengthscale, noise}; }                         // ... and ended
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

  // ---- questions ----
  bool in_flight() const { return gp_pending; }
  bool conditioned() const { return have_gp; }
  GpReady gp_ready() const { return gp_pending ? GP_IN_FLIGHT : have_gp ? GP_READY : GP_NONE; }
  bool wpca_known() const { return wpca_uncollected || have_wpca; }
  bool wpca_matches(int n_, int k_) const { return have_wpca && n == n_ && k == k_; }      // may a conditioning pass Z == NULL?
  bool warm_start(int d_) const { return vprev_d == d_; }
  bool tickets_need_reset(int slabs) const { return slabs != cnt_S || cnt_dirty; }
  RunOwn own() const { return {k, rung, have_gp, lengthscale, noise}; }

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
  void launch_may_have_died() { cnt_dirty = true; }
  void tickets_reset(int slabs) { cnt_S = slabs; cnt_dirty = false; }
  // question and transition in one: true = the caller enqueues the memset of the tickets now
  bool tickets_reset_if_needed(int slabs) { const bool need = tickets_need_reset(slabs); if (need) tickets_reset(slabs); return need; }
  inline void follow(const BatchState& b, const RunOwn& o);          // a member run after any transition of its batch
};

struct BatchState {
  ModelState m;                          // of all runs together (they advance in lock-step); k, KP and rung are each run's own
  bool fitted = false;                   // the runs carry their own hyperparameters (a lock-step fit has finished)
  bool score_enqueued = false;           // pcabo_batch_gp_condition_end_eval_begin without its _end yet
  bool imap_enqueued = false;            // pcabo_batch_inverse_map_begin without its _end yet
  bool opt_enqueued = false; int opt_restarts = 0, opt_limit = 0;      // pcabo_batch_optimize_acqf_begin without its _end yet

  // ---- questions ----
  bool begin_pending() const { return score_enqueued || opt_enqueued || imap_enqueued; }
  GpReady gp_ready() const { return m.gp_pending || begin_pending() ? GP_IN_FLIGHT : m.have_gp ? GP_READY : GP_NONE; }
  bool scorable() const { return m.gp_pending || fitted; }           // a conditioning in flight, or a fit (waited for already)
  bool anything_enqueued() const { return m.wpca_uncollected || m.n != 0; }
  bool wpca_on_host() const { return m.n != 0 && !m.wpca_uncollected; }
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
  void fit_finished() { m.gp_pending = false; m.have_gp = true; fitted = true; }
  void scoring_begun() { score_enqueued = true; }
  void scoring_ended() { score_enqueued = false; m.gp_pending = false; m.have_gp = true; }
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
// ping-pong and the ticket count.  The run's own: RunOwn.  A member never has a conditioning or a wPCA of its own in flight.  Kept:
// what only calls on the member itself change (rt_stale, zn_recorded, wpca_n / wpca_d) and its dirty mark, which only a reset clears.
inline void ModelState::follow(const BatchState& b, const RunOwn& o) {
  n = b.m.n; n_base = b.m.n_base; d = b.m.d; NP = b.m.NP; kernel = b.m.kernel;
  have_wpca = b.m.have_wpca; gcur = b.m.gcur; vprev_d = b.m.vprev_d;
  cnt_S = b.m.cnt_S; cnt_dirty = cnt_dirty || b.m.cnt_dirty;
  k = o.k; KP = round_up(o.k, 4); rung = o.rung; have_gp = o.have_gp; lengthscale = o.lengthscale; noise = o.noise;
  gp_pending = false; wpca_uncollected = false;
}
