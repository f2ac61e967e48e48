// Host-side pieces of the optimisers that need no HIP: the restart group (a joint problem on LbfgsbDriver, csrc/lbfgsb.h), the
// restart groups of one run and the round loop over several runs, the single run's optimise call (its helper threads OptHelper /
// OptCrew / CrewCall, the packing of a round pack_active / absorb_packed, and the free-running pair of two groups free_pair, a
// template over the mailbox it posts to), the GP hyperparameter fit of one run (FitRun) and the lock-step rounds over several
// (fit_rounds), and the worker pool of a batch.  What stays in pcabo_api.hip is what needs HIP: the launches, the mailbox in
// device memory and the resident kernel's session.  Included by pcabo_api.hip (the product) and by host_selftest.cpp (the
// sanitizer builds of the Makefile: `make asan ubsan tsan` compile this header, lbfgsb.cpp and host_entry.cpp with g++ and run
// them without a GPU).
#pragma once
#include "../../include/pcabo.h"
#include "lbfgsb.h"

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

// botorch's initialize_q_batch on a state blob of torch's CPU generator, in two halves (host_entry.cpp): the n Exp(1) variates of
// the multinomial draw need no score and are drawn while the device still works; the pick from them follows the scores.  The one
// spelling of the sequence - a copy of the generator, the draw, the pick, the copy put back when nothing was picked - for
// pcabo_boltzmann_pick_rows (the two halves in a row, per row), pcabo_propose_acqf and the debug export the CPU test calls.
constexpr size_t TORCH_BLOB_BYTES = 5056;            // torch.Generator.get_state() of the CPU generator
bool torch_blob_ok(const void* blob);                // seeded, and its bookkeeping cannot read past the state words
struct AheadPick {
  AheadPick(int n, int n_pick);
  void draw(void* blob);                             // keeps what of the blob a draw can change, then draws the n variates from it
  // 0: out[n_pick] picked; 1: nothing is picked here - the std of vals[n] is not positive (equal values, or a NaN), or the largest
  // ratios tie (overflowed or underflowed weights) and their order would be torch's topk's own -: out is left alone and the blob
  // is, byte for byte, what draw() found; the caller takes torch's path
  int pick(const double* vals, double eta, int64_t* out);
  void put_back();                                   // the blob as draw() found it (the scores never came)
 private:
  int n, n_pick;
  void* blob = nullptr;
  std::vector<unsigned char> before;
  std::vector<double> q, w, ratio;
  std::vector<int> best;
};

// One restart group of one run: the joint L-BFGS-B problem of restarts q0 .. q0 + nq - 1 (nq k variables) on the negated
// acquisition, and botorch's end of it (the values at the clamped end points).
struct RestartGroup : LbfgsbDriver {
  int q0 = 0, nq = 0, k = 0;
  std::vector<double> lo, hi, vc;      // the box per variable; the per-restart values of the cached evaluation
  void init(const double* ics, const double* bounds, int q0_, int nq_, int k_, int maxiter, int sum_order = 0) {
    q0 = q0_; nq = nq_; k = k_;
    lo.resize(nq * k); hi.resize(nq * k);
    for (int j = 0; j < nq; ++j)
      for (int c = 0; c < k; ++c) { lo[j * k + c] = bounds[c]; hi[j * k + c] = bounds[k + c]; }
    LbfgsbDriver::init(nq * k, ics + (size_t)q0 * k, lo.data(), hi.data(), sum_order, maxiter);   // (columnwise_clamp)
  }
  // the evaluation at x: values hVal[row .. row + nq), gradients behind hGrad + row k (of the acquisition, maximised); false: a NaN
  // in the gradient (nothing recorded)
  bool absorb(const double* hVal, const double* hGrad, int row) {
    double fs = 0.0;
    bool nan = false;
    for (int j = 0; j < nq; ++j) fs += hVal[row + j];
    for (int t = 0; t < nq * k; ++t) {
      const double gv = -hGrad[(size_t)row * k + t];
      if (gv != gv) nan = true;
      g[t] = gv;
    }
    if (nan) return false;
    LbfgsbDriver::absorb(-fs);
    vc.assign(hVal + row, hVal + row + nq);
    return true;
  }
};

// The restart groups of one run in one optimise call: restarts q0 .. q0 + batch_limit - 1 per group, and the run's host block
// (xq: the points the device reads, val / grad: the values and gradients it writes back; row q = restart q).
struct RunRestarts {
  std::vector<RestartGroup> grp;
  int status = PCABO_OK;               // PCABO_ERR_NAN once a gradient had a NaN (run_rounds then leaves the run alone)
  double* xq = nullptr;
  const double *val = nullptr, *grad = nullptr;
  void init(const double* ics, const double* bounds, int num_restarts, int batch_limit, int k, int maxiter, int sum_order = 0) {
    grp.resize((num_restarts + batch_limit - 1) / batch_limit);
    for (size_t gi = 0; gi < grp.size(); ++gi) {
      const int q0 = (int)gi * batch_limit;
      grp[gi].init(ics, bounds, q0, std::min(batch_limit, num_restarts - q0), k, maxiter, sum_order);
    }
    status = PCABO_OK;
  }
  void bind(double* xq_, const double* val_, const double* grad_) { xq = xq_; val = val_; grad = grad_; }
  // botorch's end: the end points clamped into the box, into cand.  A group whose clamped end point is its last evaluated point
  // copies that evaluation's values (the ones a launch there would give) into vals; any other is handed to redo(group), which must
  // evaluate it there.  Returns the number of groups handed on.
  template <class Redo> int end_points(double* cand, double* vals, Redo&& redo) {
    int n = 0;
    for (RestartGroup& rg : grp) {
      if (rg.end_point(cand + (size_t)rg.q0 * rg.k)) std::copy(rg.vc.begin(), rg.vc.end(), vals + rg.q0);   // (LbfgsbDriver: clamp, compare, count)
      else { redo(rg); ++n; }
    }
    return n;
  }
  int end_points(double* cand, double* vals) { return end_points(cand, vals, [](const RestartGroup&) {}); }
  // niter, nfev, warnflag, task of group gi into info[4 (slot0 + gi) .. + 3] (info may be null); true: some group failed
  // (warnflag 2)
  bool report(int* info, size_t slot0) const {
    bool any = false;
    for (size_t gi = 0; gi < grp.size(); ++gi) {
      const RestartGroup& rg = grp[gi];
      const int wf = rg.opt.warnflag();
      if (info) { int* o = info + 4 * (slot0 + gi); o[0] = rg.niter; o[1] = rg.nfev; o[2] = wf; o[3] = rg.opt.task(); }
      if (wf == 2) any = true;
    }
    return any;
  }
};

// Launch-table entries as the acquisition kernels read them: a restart group, or one query
inline unsigned group_entry(int run, int q0, int nq) { return ((unsigned)run << 16) | ((unsigned)q0 << 8) | (unsigned)nq; }
inline unsigned query_entry(int run, int q) { return ((unsigned)run << 16) | (unsigned)q; }

// The restart rounds of the runs order[..] (indices into runs) until no group wants an evaluation.  A round advances every
// active group of every run whose status is PCABO_OK (runs in the given order, groups by index), copies its point into its
// run's xq and hands it to stage(run, group); eval() then evaluates what was staged since its last call and returns PCABO_OK or
// an error, which ends the rounds and is returned.  Each staged group absorbs its run's val / grad; a NaN in a gradient sets
// the run's status to PCABO_ERR_NAN.  Only the runs listed are touched: workers may drive disjoint lists of one runs array.
template <class Stage, class Eval>
int run_rounds(RunRestarts* runs, const std::vector<int>& order, Stage&& stage, Eval&& eval) {
  std::vector<std::pair<RunRestarts*, RestartGroup*>> pend;
  size_t ng = 0;
  for (int b : order) ng += runs[b].grp.size();
  pend.reserve(ng);
  for (;;) {
    pend.clear();
    for (int b : order) {
      RunRestarts& run = runs[b];
      if (run.status != PCABO_OK) continue;
      for (RestartGroup& rg : run.grp) {
        if (!rg.advance()) continue;
        std::memcpy(run.xq + (size_t)rg.q0 * rg.k, rg.x.data(), rg.x.size() * sizeof(double));
        stage(b, rg);
        pend.push_back({&run, &rg});
      }
    }
    if (pend.empty()) return PCABO_OK;
    const int rc = eval();
    if (rc != PCABO_OK) return rc;
    for (auto& pe : pend)
      if (!pe.second->absorb(pe.first->val, pe.first->grad, pe.second->q0)) pe.first->status = PCABO_ERR_NAN;
  }
}

// ---- the single run's optimise call (pcabo_optimize_acqf; DESIGN.md "Multi-start optimiser") ------------------------------------
// One helper thread for the restart groups the calling thread does not step itself.  It lives as long as its context (creating
// and joining a thread per call cost ~0.1 ms per BO iteration), sleeps on a condition variable between calls and spin-waits on
// `go` only while a call is active.  `go`/`done` are monotonic round counters.
struct OptHelper {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<unsigned> go{0}, done{0};
  std::atomic<bool> quit{false}, active{false};
  std::function<void()> fn;          // written by the caller only while the helper is idle (done == go)
  void run() {
    unsigned seen = 0;
    while (true) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return active.load(std::memory_order_acquire) || quit.load(std::memory_order_acquire); });
      }
      if (quit.load(std::memory_order_acquire)) return;
      while (active.load(std::memory_order_acquire)) {
        const unsigned cur = go.load(std::memory_order_acquire);
        if (cur == seen) { __builtin_ia32_pause(); continue; }
        seen = cur;
        fn();
        done.store(cur, std::memory_order_release);
      }
    }
  }
  void start() { if (!th.joinable()) th = std::thread([this] { run(); }); }
  void begin(std::function<void()> f) {
    start();
    fn = std::move(f);
    { std::lock_guard<std::mutex> lk(mu); active.store(true, std::memory_order_release); }
    cv.notify_one();
  }
  void end() { active.store(false, std::memory_order_release); }
  // Leave the condition variable now and spin, before the call that will need the helper is there: `go` has not moved, so
  // nothing runs until a later begin() has given it its work and post() has asked for it.  Only while the helper is idle.  Followed
  // by begin() + end() of a call, or by end() alone when no call came.
  void wake() { if (!active.load(std::memory_order_acquire)) begin([] {}); }
  void shutdown() {
    if (!th.joinable()) return;
    { std::lock_guard<std::mutex> lk(mu); quit.store(true, std::memory_order_release); active.store(false, std::memory_order_release); }
    cv.notify_one();
    th.join();
  }
  // hand the helper its next piece of work / wait until it has done it (the helper must be idle: done == go)
  unsigned post() {
    const unsigned ticket = go.load(std::memory_order_relaxed) + 1;
    go.store(ticket, std::memory_order_release);
    return ticket;
  }
  void wait(unsigned ticket) const { while (done.load(std::memory_order_acquire) != ticket) __builtin_ia32_pause(); }
};

// The helpers of a context: one, and up to five more once a call has many restart groups.
struct OptCrew {
  OptHelper helper;
  std::vector<std::unique_ptr<OptHelper>> more;
  // The first helper spins from here until the guard goes (OptHelper::wake): its wake-up latency then lies beside the wait that
  // precedes an optimise call, not in front of the call's first round.  A CrewCall inside the guard's life takes the helper over.
  struct Awake {
    OptHelper& h;
    explicit Awake(OptCrew& c) : h(c.helper) { h.wake(); }
    Awake(const Awake&) = delete;
    ~Awake() { h.end(); }
  };
  void shutdown() {
    helper.shutdown();
    for (auto& h : more) h->shutdown();
    more.clear();
  }
};

// The stepping threads of ONE call.  The groups are independent between evaluations: thread t of T steps the groups t, t + T, ...
// (the calling thread is t = 0, helper i is t = i + 1), hand-off through the helpers' round counters, spin-waiting.  Two threads
// up to 11 groups.  With many groups (the stress configuration: 256 restarts = 52 joint problems of up to 5 x 78 variables) two
// threads spend longer on the state machines than the device on the evaluations (90-150 us against 100-180 us per round): then
// up to five more helpers share the groups.  One group: no helper at all.
// pending[gi] (char, not vector<bool>: groups are touched from several threads): the free-running pair below left group gi
// waiting for the evaluation of its point, so it is not stepped again before that evaluation.
inline int stepping_threads(int ngroups) { return ngroups >= 12 ? std::min(7, 1 + ngroups / 8) : 2; }
struct CrewCall {
  std::vector<RestartGroup>& grp;
  std::vector<char>& pending;
  const int ngroups, T;                  // T: threads that step groups, the caller included
  OptHelper* hs[6];                      // hs[i] steps the groups i + 1 (mod T)
  int nh = 0;
  CrewCall(OptCrew& crew, RunRestarts& run, std::vector<char>& pending_)
      : grp(run.grp), pending(pending_), ngroups((int)run.grp.size()), T(stepping_threads((int)run.grp.size())) {
    if (T > 2) while ((int)crew.more.size() < T - 2) crew.more.emplace_back(new OptHelper());
    if (ngroups > 1) hs[nh++] = &crew.helper;
    for (int i = 0; i < T - 2; ++i) hs[nh++] = crew.more[i].get();
    for (int i = 0; i < nh; ++i) hs[i]->begin(share(i + 1));
  }
  CrewCall(const CrewCall&) = delete;
  ~CrewCall() { for (int i = 0; i < nh; ++i) hs[i]->end(); }
  void advance(int gi) {
    if (pending[gi]) pending[gi] = 0;
    else grp[gi].advance();
  }
  void step_share(int first) { for (int gi = first; gi < ngroups; gi += T) advance(gi); }
  std::function<void()> share(int first) { return [this, first] { step_share(first); }; }
  // every group advances until it needs f, g at its x (or stops)
  void advance_all() {
    unsigned tickets[6];
    for (int i = 0; i < nh; ++i) tickets[i] = hs[i]->post();
    step_share(0);
    for (int i = 0; i < nh; ++i) hs[i]->wait(tickets[i]);
  }
  // f1 on the first helper beside f0 on the calling thread, once (between two advance_all: the helper is idle)
  template <class F1, class F0> void beside(F1&& f1, F0&& f0) {
    OptHelper& hp = *hs[0];
    hp.fn = std::forward<F1>(f1);
    const unsigned ticket = hp.post();
    f0();
    hp.wait(ticket);
    hp.fn = share(1);
  }
};

// The points of the active groups, contiguously and in group order, into the run's xq; qoff[gi] = the first query slot of group
// gi there, -1: not active.  Returns the number of points.  (run_rounds keeps each group at its q0 instead: a batch's launch
// table names the slots, a single run's launch takes the first nq.)
inline int pack_active(RunRestarts& run, std::vector<int>& qoff) {
  int nq = 0;
  for (size_t gi = 0; gi < run.grp.size(); ++gi) {
    const RestartGroup& rg = run.grp[gi];
    qoff[gi] = -1;
    if (!rg.active) continue;
    qoff[gi] = nq;
    std::memcpy(run.xq + (size_t)nq * rg.k, rg.x.data(), rg.x.size() * sizeof(double));
    nq += rg.nq;
  }
  return nq;
}
// ... and their evaluation, from the run's val / grad at the same slots, into the groups; false: a NaN in a gradient
inline bool absorb_packed(RunRestarts& run, const std::vector<int>& qoff) {
  for (size_t gi = 0; gi < run.grp.size(); ++gi)
    if (qoff[gi] >= 0 && !run.grp[gi].absorb(run.val, run.grad, qoff[gi])) return false;
  return true;
}

// The two restart groups of a call free of each other, on an evaluator that answers each query slot by itself (the resident
// acquisition kernel): each group has its own slots, control words and round counter, so each thread drives its own group
// (post - wait - L-BFGS-B step) without meeting the other: a round does not wait for the slower of the two steps and there is no
// hand-off between the threads.  Same evaluations, same order per group.  Group 1 runs on the crew's first helper, group 0 on the
// calling thread; both groups want the evaluation of their x when it starts and sit at their q0 of the run's val / grad.
// The mailbox:
//   post(q0, nq, x, tag)   the nq k coordinates of the queries q0 .. and their nq "evaluate" controls, under tag
//   tag_of(q)              the tag query q's results were published under (acquire: the results are visible behind it)
//   leave(q0, nq, tag)     "leave for good" for the queries q0 .., under tag
// Round r of a group (r = 1, 2, ...) carries the tag seq0 + r; a group leaves at seq0 + r + 1 (used[gi]: the tags it has taken,
// the leave included).  An answer later than `timeout` ends both groups (checked every 4096 spins, with the other group's abort);
// a group that stops while its point is not evaluated sets pending[gi] and the caller's lock-step rounds finish the call.
struct FreePair {
  bool timed_out[2] = {false, false}, got_nan[2] = {false, false};
  bool slow_first[2] = {false, false};   // the first answer took longer than `slow`: the evaluator was not ready at once
  unsigned long long used[2] = {0, 0};
};
template <class Mailbox>
void free_group(RestartGroup& rg, int gi, Mailbox& mb, const double* val, const double* grad, unsigned long long seq0,
                std::atomic<int>& abort_flag, char& pending, FreePair& out, std::chrono::nanoseconds timeout,
                std::chrono::nanoseconds slow) {
  const int q0 = rg.q0, nq = rg.nq;
  unsigned long long r = 0;
  for (;;) {
    if (abort_flag.load(std::memory_order_relaxed)) { pending = 1; break; }
    const unsigned long long tag = seq0 + (++r);
    mb.post(q0, nq, rg.x.data(), tag);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long spins = 0;
    bool ok = true;
    for (int j = 0; j < nq && ok; ++j) {
      while (mb.tag_of(q0 + j) != tag) {
        if ((++spins & 0xFFF) == 0) {
          if (abort_flag.load(std::memory_order_relaxed)) { ok = false; break; }
          if (std::chrono::steady_clock::now() - t0 > timeout) {
            out.timed_out[gi] = true; abort_flag.store(1, std::memory_order_relaxed); ok = false; break;
          }
        }
      }
    }
    if (!ok) { pending = 1; break; }
    if (r == 1 && std::chrono::steady_clock::now() - t0 > slow) out.slow_first[gi] = true;
    if (!rg.absorb(val, grad, q0)) { out.got_nan[gi] = true; abort_flag.store(1, std::memory_order_relaxed); break; }
    if (!rg.advance()) break;
  }
  // this group's slots may go (the evaluator waits for round r + 1 of their own count)
  mb.leave(q0, nq, seq0 + r + 1);
  out.used[gi] = r + 1;
}
template <class Mailbox>
FreePair free_pair(CrewCall& crew, RunRestarts& run, Mailbox& mb, unsigned long long seq0,
                   std::chrono::nanoseconds timeout = std::chrono::seconds(3),
                   std::chrono::nanoseconds slow = std::chrono::milliseconds(1)) {
  assert(run.grp.size() == 2 && crew.nh >= 1);
  FreePair out;
  std::atomic<int> abort_flag{0};
  const auto drive = [&](int gi) {
    free_group(run.grp[gi], gi, mb, run.val, run.grad, seq0, abort_flag, crew.pending[gi], out, timeout, slow);
  };
  crew.beside([&] { drive(1); }, [&] { drive(0); });
  return out;
}

// ---- GP hyperparameter fit (DESIGN.md "GP hyperparameter fit") ---------------------------------------------------------------
// theta = {noise s2, mean constant c, rho_1 .. rho_m}: m raw lengthscales, lengthscale = softplus(rho) as torch computes it
// (threshold 20).  Two forms of the model: the shared lengthscale (m = 1, pcabo_gp_mll / pcabo_gp_fit and the batch) and ARD, one
// lengthscale per input (m = k, pcabo_gp_mll_ard / pcabo_gp_fit_ard).  The scalar model is the ARD layout with one rho; the forms
// differ in one rule, fit_rho_lower, and in nothing else on the host.
constexpr int FIT_ARD_MAXVAR = 2 + 128;  // 2 + the largest reduced dimension (PCABO_MAXD)
inline double softplus_host(double x) { return x > 20.0 ? x : std::log1p(std::exp(x)); }
inline bool lengthscale_ok(double rho) {
  const double ls = softplus_host(rho);
  return ls > 0.0 && std::isfinite(ls);
}
inline bool mll_theta_ok(const double* theta, int m) {
  const double s2 = theta[0], c = theta[1];
  if (!(s2 > 0.0 && std::isfinite(s2) && std::isfinite(c))) return false;
  for (int j = 0; j < m; ++j)
    if (!lengthscale_ok(theta[2 + j])) return false;
  return true;
}
// Rule 1, the fit's lower bound on rho.  ARD bounds every rho_c by ln 2^-40, a lengthscale of 2^-40 of the Normalize range, which
// is where k_zstats holds a folded range (below it the device no longer evaluates the model at rho_c, and K = I to rounding
// anyway).  The flat directions of the irrelevant inputs give L-BFGS-B trial steps of thousands in rho_c; as a bound, the line
// search's longest step ends there and backtracks, where softplus(rho_c) = 0 would end the fit by the domain stop.  No fitted model
// is near it.  The shared lengthscale is not bounded.
constexpr double FIT_ARD_RHO_MIN = -27.725887222397812;
inline double fit_rho_lower(bool ard) { return ard ? FIT_ARD_RHO_MIN : -INFINITY; }
// d softplus / d rho, of the softplus the loss evaluates: above the threshold softplus_host takes the linear branch, ls = rho, so the
// derivative there is 1 (torch's rule), the sigmoid below.  Both forms of the model share it.  (The shared lengthscale used to
// take the sigmoid throughout, 1 - e^-rho above the threshold: a gradient 1.25e-9 short of its loss's at rho = 20.5, which the
// extended reference of tests/mll_reference.py sees at 10^2 to 10^5 of its units on the device.)
inline double softplus_slope(double rho) { return rho > 20.0 ? 1.0 : 1.0 / (1.0 + std::exp(-rho)); }
// Loss and gradient of one evaluation, assembled on the host (the prior on s2 and the chain rule through softplus are host
// arithmetic): h = {sum log L_ii, y_s^T alpha, sum alpha, alpha^T alpha, tr K^-1, S_1 .. S_m} of a state conditioned at theta,
// S_c = sum_ij W_ij dK_ij/dlog l_c (m = 1: S = sum W dK/dlog l; the S_c of equal rho add up to it).  The same arithmetic for
// both forms of the model: only m tells them apart here.
inline void mll_assemble(const double* h, int n, int m, const double* theta, double* loss, double* grad) {
  const double s2 = theta[0];
  const double LOG2PI = 1.8378770664093453;
  const double lnz = std::log(s2), u = lnz + 4.0;
  const double log_n = -0.5 * h[1] - h[0] - 0.5 * n * LOG2PI;
  const double log_prior = -lnz - 0.5 * LOG2PI - 0.5 * u * u;              // LogNormal(-4, 1) at s2
  *loss = -(log_n + log_prior) / n;
  if (grad) {
    grad[0] = -((0.5 * (h[3] - h[4])) + (-1.0 - u) / s2) / n;
    grad[1] = -h[2] / n;
    for (int j = 0; j < m; ++j) {
      const double rho = theta[2 + j], ls = softplus_host(rho);
      const double sig = softplus_slope(rho);
      grad[2 + j] = -(0.5 * h[5 + j] * sig / ls) / n;
    }
  }
}

// The fit of one run: scipy.optimize.minimize(method="L-BFGS-B") with its defaults (LbfgsbDriver: the start clipped into the box,
// scipy's memoisation of the last point, its limits) and the rules around it.  A run is STEPPING (its driver asks for evaluations),
// at its END point (one more evaluation: the result is not the last point evaluated), RESTING at its result, or OUT (never
// started, or failed: status says why).  A trial theta outside the model's domain (a line-search step so long that softplus(rho)
// underflows to 0, a non-finite value) and one the factorisation cannot take end the fit abnormally at the last accepted iterate
// (warnflag 2, task PCABO_FIT_TASK_*); when that theta is the start itself the run fails (PCABO_ERR_ARG / PCABO_ERR_NOT_PD).
// A run holds nvar = 2 + m variables of FIT_ARD_MAXVAR; runs of both forms and of different m step side by side in fit_rounds.
struct FitRun {
  enum { STEPPING, END, RESTING, OUT };
  LbfgsbDriver fit;
  int state = OUT, status = PCABO_ERR_ARG, stop_task = 0;
  int nvar = 3;
  bool ard = false;
  double xr[FIT_ARD_MAXVAR] = {}, fr = 0.0;   // the result (nvar doubles) and the loss there
  const double* h = nullptr;           // where the evaluator leaves the sums of this run (bind)
  void bind(const double* h_) { h = h_; }
  void init(const double* theta0, int m = 1, bool ard_ = false) {
    assert(m >= 1 && 2 + m <= FIT_ARD_MAXVAR && (ard_ || m == 1));
    nvar = 2 + m; ard = ard_;
    state = OUT; status = PCABO_ERR_ARG; stop_task = 0;
    for (int j = 0; j < m; ++j)                          // a start with a lengthscale outside the domain fails; it is not clipped
      if (!lengthscale_ok(theta0[2 + j])) return;
    double lower[FIT_ARD_MAXVAR], upper[FIT_ARD_MAXVAR];
    std::fill(lower, lower + nvar, -INFINITY);
    std::fill(upper, upper + nvar, INFINITY);
    lower[0] = 1e-4;
    std::fill(lower + 2, lower + nvar, fit_rho_lower(ard));
    fit.keep_accepted = true;                            // scipy's defaults and limits, the published order
    fit.init(nvar, theta0, lower, upper);
    state = STEPPING; status = PCABO_OK;
  }
  bool theta_ok(const double* th) const { return mll_theta_ok(th, nvar - 2); }
  void assemble(int n, const double* th, double* f, double* g) const { mll_assemble(h, n, nvar - 2, th, f, g); }
  // The theta to evaluate next, or null: the run has its result, or is out.
  const double* next() {
    if (state == STEPPING && !fit.advance()) finish();
    if (state == STEPPING && !theta_ok(fit.x.data())) {
      if (fit.have_cache) { stop_task = PCABO_FIT_TASK_DOMAIN; finish(); }
      else { state = OUT; status = PCABO_ERR_ARG; }      // (the start itself)
    }
    return state == STEPPING ? fit.x.data() : (state == END ? xr : nullptr);
  }
  // Where a run that wants no evaluation rides along in a lock-step round: at its result, or null (out: the shared model)
  const double* rest() const { return state == RESTING ? xr : nullptr; }
  // The outcome of evaluating the theta handed out last (next() or rest()): st, and on PCABO_OK the sums in h
  void took(int st, int n) {
    if (state == OUT) return;
    if (state == STEPPING && st == PCABO_ERR_NOT_PD && fit.have_cache) {   // a trial theta, not the start: stop, keep the last iterate
      stop_task = PCABO_FIT_TASK_NOT_PD;
      finish();
      return;
    }
    if (st != PCABO_OK) { state = OUT; status = st; return; }
    if (state == STEPPING) {
      double f = 0.0;
      assemble(n, fit.x.data(), &f, fit.g.data());
      fit.absorb(f);
    } else if (state == END) {
      assemble(n, xr, &fr, nullptr);
      state = RESTING;
    }
  }
  // niter, nfev, warnflag, task of a run whose status is PCABO_OK
  void report(int* info) const {
    info[0] = fit.niter; info[1] = fit.nfev;
    info[2] = stop_task ? 2 : fit.opt.warnflag();
    info[3] = stop_task ? stop_task : fit.opt.task();
  }

 private:
  // the optimiser has stopped (it restores the last iterate itself) or met a theta it cannot take (the last accepted iterate):
  // the state is left conditioned at the result, so one more evaluation unless the result is the last point evaluated (after a
  // NOT_PD stop in any case: the state holds the trial theta's failed factorisation)
  void finish() {
    const size_t bytes = (size_t)nvar * sizeof(double);
    std::memcpy(xr, stop_task ? fit.xacc.data() : fit.x.data(), bytes);
    fr = fit.fc;
    state = (stop_task == PCABO_FIT_TASK_NOT_PD || !fit.have_cache || std::memcmp(xr, fit.xc.data(), bytes) != 0) ? END : RESTING;
  }
};

// The rounds of the runs' fits in lock-step until no run wants an evaluation: eval(th, st) evaluates run b at th[b] (null: a run
// that is out), leaves its sums where the run was bound and its outcome in st[b], and returns PCABO_OK or an error, which
// ends the rounds and is returned.  n: the number of training points of every run.
template <class Eval>
int fit_rounds(std::vector<FitRun>& runs, int n, Eval&& eval) {
  std::vector<const double*> th(runs.size(), nullptr);
  std::vector<int> st(runs.size(), PCABO_OK);
  for (;;) {
    int pending = 0;
    for (size_t b = 0; b < runs.size(); ++b) {
      const double* t = runs[b].next();
      if (t) ++pending;
      th[b] = t ? t : runs[b].rest();
    }
    if (pending == 0) return PCABO_OK;
    const int rc = eval(th, st.data());
    if (rc != PCABO_OK) return rc;
    for (size_t b = 0; b < runs.size(); ++b) runs[b].took(st[b], n);
  }
}

// Worker pool of a batch: the calling thread is worker 0, n - 1 persistent threads are workers 1..n-1 (sleeping between
// calls, woken per call).  With one worker nothing leaves the calling thread (PCABO_BATCH_THREADS=1: profiler runs).
struct GangPool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv, cv_done;
  std::function<void(int)> fn;
  unsigned epoch = 0;
  int pending = 0;
  bool quit = false;
  void start(int n) {
    const unsigned epoch0 = epoch;                         // (a restarted pool must not take the last call for a new one)
    for (int i = 1; i < n; ++i)
      th.emplace_back([this, i, epoch0] {
        unsigned seen = epoch0;
        for (;;) {
          std::function<void(int)> f;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return quit || epoch != seen; });
            if (quit) return;
            seen = epoch;
            f = fn;
          }
          f(i);
          { std::lock_guard<std::mutex> lk(mu); if (--pending == 0) cv_done.notify_all(); }
        }
      });
  }
  void run(std::function<void(int)> f) {                   // every worker runs f(worker index); returns when all are done
    {
      std::lock_guard<std::mutex> lk(mu);
      fn = f;
      pending = (int)th.size();
      ++epoch;
    }
    cv.notify_all();
    f(0);
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
  }
  void shutdown() {
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv.notify_all();
    for (auto& t : th) if (t.joinable()) t.join();
    th.clear();
    quit = false;
  }
};

// Row O on the host, x = z Ck + m_w + mu_x (PCA_BO.py:427), with the bits of k_inverse_map: per coordinate j the device runs
// s = fma(z[c], comps[c][j], s) from s = 0 with c ascending (its `s += z[c] * comps[c][j]` compiles to one fused multiply-add per
// term), then (s + pca_mean[j]) + data_mean[j] in two plain additions.  A fused multiply-add rounds once wherever it runs, so
// the host's chain gives the same x; the loops are turned round (c outside, j along the row of comps) which changes no
// coordinate's order.  x doubles as the accumulator.  With the FMA instruction set the inner loop is a vector fma; without it
// std::fma computes the same correctly rounded result term by term.
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define PCABO_HOST_FMA_ISA 1
__attribute__((target("fma"))) inline void inverse_map_chain_fma(const double* z, const double* comps, int k, int d, double* x) {
  for (int c = 0; c < k; ++c) {
    const double zc = z[c];
    const double* row = comps + (size_t)c * d;
    for (int j = 0; j < d; ++j) x[j] = __builtin_fma(zc, row[j], x[j]);
  }
}
#endif
inline void inverse_map_chain(const double* z, const double* comps, int k, int d, double* x) {
  for (int c = 0; c < k; ++c) {
    const double zc = z[c];
    const double* row = comps + (size_t)c * d;
    for (int j = 0; j < d; ++j) x[j] = std::fma(zc, row[j], x[j]);
  }
}
inline void inverse_map_host(const double* z, const double* comps, const double* pca_mean, const double* data_mean, int k, int d,
                             double* x, bool allow_isa = true) {
  for (int j = 0; j < d; ++j) x[j] = 0.0;
#ifdef PCABO_HOST_FMA_ISA
  static const bool have_fma = __builtin_cpu_supports("fma");
  if (allow_isa && have_fma) inverse_map_chain_fma(z, comps, k, d, x);
  else
#endif
    inverse_map_chain(z, comps, k, d, x);
  for (int j = 0; j < d; ++j) x[j] = (x[j] + pca_mean[j]) + data_mean[j];
}
