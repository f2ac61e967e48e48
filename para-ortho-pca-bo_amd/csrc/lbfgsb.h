// Host-side limited-memory BFGS with box bounds (L-BFGS-B 3.0: Byrd, Lu, Nocedal, Zhu 1995;
// Morales & Nocedal 2011), reverse-communication form.
//
// The reference reaches this algorithm through botorch.optimize_acqf -> gen_candidates_scipy ->
// scipy.optimize.minimize(method="L-BFGS-B") (/root/reference/Algorithms/BayesianOptimization/
// PCA_BO.py:607-614).  This is a from-scratch restatement of the published algorithm (generalised
// Cauchy point, subspace minimisation with the 3.0 projection step, More-Thuente line search
// dcsrch/dcstep, compact L-BFGS matrices) written so that, fed the same f/g values, it takes the
// same iterates as scipy's implementation; tests/test_lbfgsb_vs_scipy.py pins it against scipy.
#pragma once
#include <vector>
#include "lb_linesearch.h"

#define LBFGSB_MAXM 32   // largest history length supported (scipy's default is 10)

enum {
  LBFGSB_START = 0,
  LBFGSB_NEW_X = 1,        // an iteration finished; caller may stop() or call step() again
  LBFGSB_FG = 3,           // caller must evaluate f and g at x, then call step() again
  LBFGSB_CONV_PG = 40,     // CONVERGENCE: NORM OF PROJECTED GRADIENT <= PGTOL
  LBFGSB_CONV_F = 41,      // CONVERGENCE: REL_REDUCTION_OF_F <= FACTR*EPSMCH
  LBFGSB_STOP_ITER = 50,   // STOP: TOTAL NO. OF ITERATIONS REACHED LIMIT   (set by the caller)
  LBFGSB_STOP_FUN = 51,    // STOP: TOTAL NO. OF F,G EVALUATIONS EXCEEDS LIMIT (set by the caller)
  LBFGSB_ABNORMAL = 70,    // ABNORMAL TERMINATION IN LNSRCH
  LBFGSB_ERROR = 90        // invalid input (l > u, ...)
};

// Branch counters (tests/test_lbfgsb_branches_cpu.py, tests/test_gpu_lbfgsb_branches.py): which branches of the step a run took.
// Plain integers, one increment per routine call or event; they take part in no floating-point operation.
#define LBFGSB_BRANCH_LIST(X)                                                                                                   \
  X(start_conv_pg) X(conv_pg) X(conv_f) X(stop_iter) X(abnormal)                                                                \
  X(update_skipped) X(update_scaled_step) X(history_wrap)                                                                       \
  X(cauchy_first_iter) X(cauchy_start_on_bound) X(cauchy_break_crossed) X(cauchy_all_at_bounds) X(cauchy_ties)                  \
  X(freev_enter) X(freev_leave) X(formk_skipped) X(subsm_skipped_nfree0) X(subsm_touched_bound) X(subsm_truncated)              \
  X(ls_backtracked) X(ls_ascent) X(ls_failed_restart)                                                                           \
  X(reset_after_cauchy) X(reset_after_formk) X(reset_after_subsm) X(reset_after_formt)                                          \
  X(fixed_variable) X(cache_hit) X(endpoint_reevaluated) X(evaluations)
enum LbfgsbBranch {
#define LBFGSB_BRANCH_ENUM(name) LBB_##name,
  LBFGSB_BRANCH_LIST(LBFGSB_BRANCH_ENUM)
#undef LBFGSB_BRANCH_ENUM
  LBB_COUNT
};
const char* lbfgsb_branch_name(int which);   // "start_conv_pg", ... (null beyond LBB_COUNT)

// 0: scalar O(m n) loops, 1: the default (AVX2 where available); same iterates either way.  Returns the previous setting.
int lbfgsb_set_vector_kernels(int enabled);

class Lbfgsb {
 public:
  // lower/upper may be null (unbounded); +-inf entries mean "no bound on that side".  sum_order: the order of the sums over the
  // variables - 0 the published order (scipy's iterates), 1 the 64-lane tree order the device-resident optimiser steps in
  // (see lbfgsb.cpp).
  void init(int n, int m, const double* lower, const double* upper, double factr, double pgtol, int maxls, int sum_order);
  int step(double* x, double* f, double* g);
  void stop(int code) { task_ = code; }
  int task() const { return task_; }
  // scipy's warnflag: 0 converged, 1 iteration/evaluation limit, 2 anything else
  int warnflag() const {
    if (task_ == LBFGSB_CONV_PG || task_ == LBFGSB_CONV_F) return 0;
    if (task_ == LBFGSB_STOP_ITER || task_ == LBFGSB_STOP_FUN) return 1;
    return 2;
  }
  int iterations() const { return iter_; }
  // the branch counters since init (LBB_COUNT of them); count() is for the driver's own events
  const unsigned* branches() const { return branch_; }
  void count(int which, unsigned by = 1) { branch_[which] += by; }
  // v clamped into the bounds of variable i (the end point botorch evaluates)
  double clamped(int i, double v) const {
    if (nbd_[i] != 0 && nbd_[i] <= 2 && v < l_[i]) v = l_[i];
    if (nbd_[i] >= 2 && v > u_[i]) v = u_[i];
    return v;
  }

 private:
  // problem
  int n_ = 0, m_ = 0, maxls_ = 20;
  unsigned branch_[LBB_COUNT] = {};
  int sum_order_ = 0;        // 0: the published order, 1: the 64-lane tree order (the device optimiser's twin)
  double factr_ = 1e7, pgtol_ = 1e-5;
  std::vector<double> l_, u_;
  std::vector<int> nbd_;
  // L-BFGS matrices (column-major, Fortran layout)
  std::vector<double> ws_, wy_, sy_, ss_, wt_, wn_, snd_;
  std::vector<double> wr_, sc_coef_, sc_full_;   // row-major mirror of WY|WS (stride rs_) and scratch, see lbfgsb.cpp
  std::vector<int> sc_rows_;
  int mp_ = 0, rs_ = 0;
  std::vector<double> z_, r_, d_, t_, xp_, wa_;
  std::vector<int> index_, iwhere_, indx2_;
  // scalars of mainlb
  bool prjctd_ = false, cnstnd_ = false, boxed_ = false, updatd_ = false, wrk_ = false;
  int nintol_ = 0, iback_ = 0, nskip_ = 0, head_ = 0, col_ = 0, itail_ = 0, iter_ = 0, iupdat_ = 0;
  int nseg_ = 0, nfgv_ = 0, info_ = 0, ifun_ = 0, iword_ = 0, nfree_ = 0, nact_ = 0, ileave_ = 0, nenter_ = 0;
  double theta_ = 1, fold_ = 0, tol_ = 0, dnorm_ = 0, epsmch_ = 0, gd_ = 0, stpmx_ = 0, sbgnrm_ = 0, stp_ = 0;
  double gdold_ = 0, dtd_ = 0, xstep_ = 0;
  int task_ = LBFGSB_START;
  int phase_ = 0;            // 0 start, 1 waiting for f,g at x0, 2 inside the line search, 3 after NEW_X
  LbLineSearch ls_;        // dcsrch state (lb_linesearch.h)

  void reset_memory();
  void projgr(const double* x, const double* g);
  bool active_init(double* x);
  void cauchy(const double* x, const double* g);
  void hpsolb(int n, double* t, int* iorder, int iheap);
  void bmv(const double* v, double* p);
  void freev();
  void formk();
  void cmprlb(const double* x, const double* g);
  void subsm(const double* x, const double* g);
  void lnsrlb(double* x, double f, const double* g);
  void matupd(double rr, double dr);
  void formt();
};

// scipy.optimize.minimize(method="L-BFGS-B") around Lbfgsb: what scipy's _minimize_lbfgsb does around setulb.  The start is
// clipped into the box (when both sides are given); ScalarFunction memoises the last evaluated point, so a trial point that
// repeats it (a line-search step that underflowed) is neither evaluated nor counted; an iteration ends in NEW_X; the run stops
// after maxiter iterations or once more than maxfun evaluations were made.  Use:
//   while (run.advance()) { evaluate f and the gradient at run.x, the gradient into run.g; run.absorb(f); }
struct LbfgsbDriver {
  Lbfgsb opt;
  std::vector<double> x, g;            // the point and the gradient there
  std::vector<double> xc, gc, xacc;    // the last evaluated point and its gradient; the last accepted iterate (keep_accepted)
  double f = 0.0, fc = 0.0;
  int niter = 0, nfev = 0, maxiter = 15000, maxfun = 15000;
  bool have_cache = false, active = true;
  bool keep_accepted = false;          // (set before init) track xacc: the clipped start, then x at every NEW_X
  void init(int n, const double* x0, const double* lower, const double* upper, int sum_order = 0, int maxiter = 15000,
            int maxfun = 15000, int m = 10, double factr = 1e7, double pgtol = 1e-5, int maxls = 20);
  bool advance();                      // step until f, g are needed at x (true) or the run has stopped (false)
  void absorb(double fx);              // one evaluation at x: fx, and the gradient the caller wrote into g
  // botorch's end of a run that has stopped: x clamped into the box, into c.  True: that is the last evaluated point (its values
  // are the cached evaluation's); false: it needs one more evaluation there (counted: endpoint_reevaluated)
  bool end_point(double* c);
};
