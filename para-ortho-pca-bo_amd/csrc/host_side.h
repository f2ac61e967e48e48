// Host-side pieces of the optimisers that need no HIP: the restart group (a joint problem on LbfgsbDriver, csrc/lbfgsb.h) and
// the worker pool of a batch.  Included by pcabo_api.hip (the product) and by host_selftest.cpp (the sanitizer builds of the Makefile:
// `make asan ubsan tsan` compile this header, lbfgsb.cpp and host_entry.cpp with g++ and run them without a GPU).
#pragma once
#include "lbfgsb.h"

#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

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
  // the end point clamped into the box, into the rows q0 .. q0 + nq - 1 of cand
  void end_point(double* cand) const {
    for (int t = 0; t < nq * k; ++t) cand[(size_t)q0 * k + t] = x[t] < lo[t] ? lo[t] : (x[t] > hi[t] ? hi[t] : x[t]);
  }
  // the clamped end point in cand is the last evaluated point: its values vc are the ones a launch there would give
  bool ends_on_cache(const double* cand) const {
    return have_cache && memcmp(cand + (size_t)q0 * k, xc.data(), (size_t)nq * k * sizeof(double)) == 0;
  }
  // niter, nfev, warnflag, task into info[4 slot .. 4 slot + 3] (info may be null); true: the group failed (warnflag 2)
  bool report(int* info, size_t slot) const {
    const int wf = opt.warnflag();
    if (info) { int* o = info + 4 * slot; o[0] = niter; o[1] = nfev; o[2] = wf; o[3] = opt.task(); }
    return wf == 2;
  }
};

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
