// Sanitizer driver for the host side of libpcabo (Makefile targets asan / ubsan / tsan; tests/test_host_sanitizers.py runs them).
// Everything here is CPU code of the product compiled by g++ with -fsanitize=...: csrc/lbfgsb.cpp, csrc/host_entry.cpp (the
// L-BFGS-B driver and the Sobol helpers), csrc/host_side.h (RestartGroup, RunRestarts, run_rounds, GangPool; FitRun, fit_rounds,
// mll_assemble) and csrc/lb_plan.h (the work plan of the device optimiser's passes).  The batch's round loop is the product's
// run_rounds with a stub evaluator: where the product launches an acquisition kernel and polls its flags, the workers here evaluate
// a bounded test objective on the CPU.  The GP fit is the product's FitRun / fit_rounds over a small dense GP in plain C++ that hands
// back the sums the likelihood kernels produce, in both forms of the model (test_fit_run: lock-step = alone, the NOT_PD / DOMAIN
// stops, resting runs, a shared-lengthscale run and an ARD run side by side).  The single run's optimise call is the product's
// too, without its launches: the helper threads of a call (OptCrew / CrewCall: test_crew, for every number of stepping threads
// the rule gives, two calls on the same helpers) and the free-running pair of two groups (free_pair: test_free_pair) over a
// mailbox in plain memory that a third thread answers in the resident kernel's place - both groups to their stop, a group that
// is never answered (the time-out is a parameter: milliseconds here), a NaN gradient.  No check uses more than eight threads.
// The memory of a context is csrc/ctx_layout.h's arithmetic (test_ctx_layout): no region is allocated, the offsets and every
// feature's use of a buffer are checked as numbers over a sweep of shapes.
// Exit code 0 and "host selftest ok" = every check passed; a sanitizer report aborts the process (halt_on_error).
#include "../../include/pcabo.h"
#include "host_side.h"
#include "lb_plan.h"
#include "ctx_layout.h"
#include "model_state.h"

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); ++g_fail; } } while (0)

struct Lcg {                                 // deterministic inputs (no libc rand state shared between threads)
  uint64_t s;
  explicit Lcg(uint64_t seed) : s(seed * 6364136223846793005ull + 1442695040888963407ull) {}
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }
};

// a smooth multi-modal objective with a box: f = sum (x_i - c_i)^2 (1 + 0.3 sin(3 x_i)) + 0.1 sum x_i x_{i+1}
struct Objective { std::vector<double> c; };
double fg_objective(const double* x, double* g, void* user) {
  const Objective* o = static_cast<const Objective*>(user);
  const int n = (int)o->c.size();
  double f = 0.0;
  for (int i = 0; i < n; ++i) {
    const double d = x[i] - o->c[i], s = 1.0 + 0.3 * std::sin(3.0 * x[i]);
    f += d * d * s;
    g[i] = 2.0 * d * s + d * d * 0.9 * std::cos(3.0 * x[i]);
  }
  for (int i = 0; i + 1 < n; ++i) { f += 0.1 * x[i] * x[i + 1]; g[i] += 0.1 * x[i + 1]; g[i + 1] += 0.1 * x[i]; }
  return f;
}

void test_minimize() {
  for (int nvar : {1, 2, 7, 33, 64, 65, 200}) {
    for (int variant = 0; variant < 3; ++variant) {       // scalar loops, vector kernels, the device optimiser's tree order
      pcabo_lbfgsb_set_vector_kernels(variant == 1);
      pcabo_lbfgsb_set_sum_order(variant == 2);
      Lcg r(17 + nvar);
      Objective o; o.c.resize(nvar);
      std::vector<double> x(nvar), lo(nvar), hi(nvar);
      for (int i = 0; i < nvar; ++i) { o.c[i] = 4.0 * r.uni() - 2.0; lo[i] = -1.0 - r.uni(); hi[i] = 1.0 + r.uni(); x[i] = 6.0 * r.uni() - 3.0; }
      double f = 0.0; int nit = 0, nfev = 0, task = 0;
      const int wf = pcabo_lbfgsb_minimize(nvar, x.data(), lo.data(), hi.data(), fg_objective, &o, 10, 1e7, 1e-5, 200, 15000, 20, &f, &nit, &nfev, &task);
      CHECK(wf >= 0 && wf <= 2, "warnflag %d", wf);
      CHECK(std::isfinite(f) && nfev >= 1, "f %g nfev %d", f, nfev);
      for (int i = 0; i < nvar; ++i) CHECK(x[i] >= lo[i] && x[i] <= hi[i], "x[%d] = %g outside the box", i, x[i]);
    }
  }
  pcabo_lbfgsb_set_vector_kernels(1);
  pcabo_lbfgsb_set_sum_order(0);
  // unbounded and half-bounded sides, a history longer than the default
  {
    const int nvar = 12;
    Objective o; o.c.assign(nvar, 0.5);
    std::vector<double> x(nvar, 2.0), lo(nvar, -INFINITY), hi(nvar, INFINITY);
    for (int i = 0; i < nvar; i += 3) lo[i] = 0.75;
    for (int i = 1; i < nvar; i += 3) hi[i] = 0.25;
    double f = 0.0; int nit = 0, nfev = 0, task = 0;
    const int wf = pcabo_lbfgsb_minimize(nvar, x.data(), lo.data(), hi.data(), fg_objective, &o, 17, 1e7, 1e-5, 200, 15000, 20, &f, &nit, &nfev, &task);
    CHECK(wf == 0, "half-bounded problem: warnflag %d task %d", wf, task);
  }
  CHECK(pcabo_lbfgsb_minimize(0, nullptr, nullptr, nullptr, fg_objective, nullptr, 10, 1e7, 1e-5, 1, 1, 20, nullptr, nullptr, nullptr, nullptr) == PCABO_ERR_ARG, "bad arguments accepted");
}

void test_sobol() {
  for (int k : {1, 3, 36, 89}) {
    Lcg r(5 + k);
    std::vector<int64_t> state((size_t)k * 30), ltm((size_t)k * 30 * 30), shift(k);
    for (auto& v : state) v = (int64_t)(r.uni() * 1073741824.0);
    for (auto& v : ltm) v = r.uni() < 0.5 ? 0 : 1;
    for (auto& v : shift) v = (int64_t)(r.uni() * 1073741824.0);
    CHECK(pcabo_sobol_scramble(state.data(), ltm.data(), k) == PCABO_OK, "scramble");
    for (int n : {1, 2, 512, 513}) {
      std::vector<double> lo(k, -1.5), rng(k, 3.0), out((size_t)n * k, -7.0);
      CHECK(pcabo_sobol_draw(state.data(), shift.data(), k, n, lo.data(), rng.data(), out.data()) == PCABO_OK, "draw");
      for (double v : out) CHECK(v >= -1.5 && v <= 1.5, "sample %g outside the box", v);
      CHECK(pcabo_sobol_draw(state.data(), shift.data(), k, n, nullptr, nullptr, out.data()) == PCABO_OK, "draw (unit cube)");
      for (double v : out) CHECK(v >= 0.0 && v < 1.0, "unit sample %g", v);
    }
  }
}

// torch's CPU generator restated (csrc/host_entry.cpp): state blobs of the published layout, the bit draws, the multinomial rows
// and the Boltzmann pick; all rows in one call = one call per row.
void test_torch_rng() {
  struct Blob { uint64_t seed; int32_t left, seeded; uint64_t next; uint64_t state[624]; unsigned char tail[32]; };
  const int rows = 70, n = 512, n_pick = 10;
  std::vector<Blob> blobs(rows), again;
  std::vector<double> vals((size_t)rows * n);
  for (int r = 0; r < rows; ++r) {
    Lcg g(900 + r);
    blobs[r].seed = 900 + r; blobs[r].left = 1 + (r * 37) % 624; blobs[r].seeded = 1; blobs[r].next = 624 - blobs[r].left;
    for (auto& w : blobs[r].state) w = (uint64_t)(g.uni() * 4294967296.0);
    for (auto& c : blobs[r].tail) c = 0;
    for (int i = 0; i < n; ++i) vals[(size_t)r * n + i] = r == 5 ? 1.25 : 40.0 * g.uni() - 20.0;        // row 5: all equal
  }
  again = blobs;
  std::vector<void*> ptr(rows);
  for (int r = 0; r < rows; ++r) ptr[r] = &blobs[r];
  ptr[7] = nullptr;                                                                                       // row 7: skipped
  std::vector<int64_t> out((size_t)rows * n_pick, -1), out1((size_t)rows * n_pick, -1);
  std::vector<int> flags(rows, -1), flags1(rows, -1);
  CHECK(pcabo_boltzmann_pick_rows(ptr.data(), vals.data(), rows, n, n_pick, 1.0, out.data(), flags.data()) == PCABO_OK, "pick rows");
  for (int r = 0; r < rows; ++r) {                            // one row per call
    void* p1 = r == 7 ? nullptr : (void*)&again[r];
    CHECK(pcabo_boltzmann_pick_rows(&p1, vals.data() + (size_t)r * n, 1, n, n_pick, 1.0, out1.data() + (size_t)r * n_pick, flags1.data() + r) == PCABO_OK, "pick row %d", r);
    CHECK(flags[r] == flags1[r] && flags[r] == (r == 7 ? 2 : r == 5 ? 1 : 0), "flag of row %d: %d / %d", r, flags[r], flags1[r]);
    if (flags[r] != 0) continue;
    for (int j = 0; j < n_pick; ++j) {
      CHECK(out[(size_t)r * n_pick + j] == out1[(size_t)r * n_pick + j], "row %d pick %d differs between the all-rows call and the one-row call", r, j);
      CHECK(out[(size_t)r * n_pick + j] >= 0 && out[(size_t)r * n_pick + j] < n, "row %d pick %d out of range", r, j);
    }
    CHECK(blobs[r].left == again[r].left && blobs[r].next == again[r].next && blobs[r].state[0] == again[r].state[0], "generator of row %d", r);
  }
  std::vector<int64_t> bits(2000);
  CHECK(pcabo_torch_randint2(&blobs[0], 2000, bits.data()) == PCABO_OK, "randint2");
  for (int64_t b : bits) CHECK(b == 0 || b == 1, "bit %lld", (long long)b);
  std::vector<double> w((size_t)3 * n);
  Lcg g(77);
  for (auto& v : w) v = 0.01 + g.uni();
  void* three[3] = {&blobs[1], nullptr, &blobs[2]};
  std::vector<int64_t> idx(3 * n_pick, -1);
  CHECK(pcabo_torch_multinomial_rows(three, w.data(), 3, n, n_pick, idx.data()) == PCABO_OK, "multinomial rows");
  for (int j = 0; j < n_pick; ++j) CHECK(idx[j] >= 0 && idx[j] < n && idx[n_pick + j] == -1 && idx[2 * n_pick + j] >= 0, "multinomial pick %d", j);
  blobs[3].left = 900;
  CHECK(pcabo_torch_randint2(&blobs[3], 4, bits.data()) == PCABO_ERR_ARG, "a broken blob accepted");

  // The pick in two halves (host_side.h) = pcabo_boltzmann_pick_rows: the variates drawn first, the pick from them after; a row
  // without spread (equal values, a NaN) reports 1 and the caller's copy puts the generator back byte for byte.
  for (int r : {0, 5, 11, 12}) {
    std::vector<double> row(vals.begin() + (size_t)r * n, vals.begin() + (size_t)(r + 1) * n);
    if (r == 12) row[100] = NAN;
    Blob two = again[r], rows1 = again[r];
    const Blob before = two;
    std::vector<int64_t> a(n_pick, -1), b(n_pick, -1);
    int flag1 = -1;
    void* p1 = &rows1;
    CHECK(pcabo_boltzmann_pick_rows(&p1, row.data(), 1, n, n_pick, 1.0, b.data(), &flag1) == PCABO_OK, "pick row %d again", r);
    CHECK(torch_blob_ok(&two), "blob of row %d refused", r);
    AheadPick ahead(n, n_pick);
    ahead.draw(&two);
    CHECK(memcmp(&two, &before, sizeof(Blob)) != 0, "the draw of row %d left its generator alone", r);
    ahead.put_back();                                          // the scores never came: as it was, and the same draw again
    CHECK(memcmp(&two, &before, sizeof(Blob)) == 0, "put_back of row %d", r);
    ahead.draw(&two);
    const int flag = ahead.pick(row.data(), 1.0, a.data());
    CHECK(flag == flag1 && flag == (r == 5 || r == 12 ? 1 : 0), "flag of the two halves on row %d: %d / %d", r, flag, flag1);
    if (flag == 1) {
      CHECK(memcmp(&two, &before, sizeof(Blob)) == 0, "the two halves moved the generator of a row without spread (row %d)", r);
      CHECK(memcmp(&rows1, &before, sizeof(Blob)) == 0, "a row without spread moved its generator (row %d)", r);
      for (int j = 0; j < n_pick; ++j) CHECK(a[j] == -1, "a row without spread wrote pick %d", j);
    } else {
      for (int j = 0; j < n_pick; ++j) CHECK(a[j] == b[j], "row %d pick %d: the two halves differ from the one call", r, j);
      CHECK(memcmp(&two, &rows1, sizeof(Blob)) == 0, "generator of row %d after the two halves", r);
    }
  }
  // the one blob checker: seeded, left in [1, 624], and left == 1 or next + left <= 625 - at all four doors
  struct { int left, seeded; uint64_t next; bool ok; } shapes[] = {
      {1, 1, 0, true}, {1, 1, 9999, true}, {624, 1, 1, true}, {624, 1, 2, false}, {2, 1, 623, true}, {2, 1, 624, false},
      {0, 1, 0, false}, {625, 1, 0, false}, {300, 0, 10, false}, {300, 1, 325, true}, {300, 1, 326, false},
      {300, 1, ~0ull - 298, false} /* next + left wraps to 1 */, {2, 1, ~0ull, false}, {624, 1, ~0ull - 622, false}, {1, 1, ~0ull, true}};
  for (const auto& sh : shapes) {
    Blob t = again[1];
    t.left = sh.left; t.seeded = sh.seeded; t.next = sh.next;
    void* pt = &t;
    int fl = -1;
    CHECK(torch_blob_ok(&t) == sh.ok, "checker on left %d next %llu", sh.left, (unsigned long long)sh.next);
    if (sh.ok) continue;                 // (an accepted shape is drawn from in the cases above)
    CHECK(pcabo_torch_randint2(&t, 4, bits.data()) == PCABO_ERR_ARG, "randint2 took left %d next %llu", sh.left, (unsigned long long)sh.next);
    CHECK(pcabo_boltzmann_pick_rows(&pt, vals.data(), 1, n, n_pick, 1.0, out1.data(), &fl) == PCABO_ERR_ARG, "pick rows took left %d", sh.left);
    CHECK(pcabo_torch_multinomial_rows(&pt, w.data(), 1, n, n_pick, idx.data()) == PCABO_ERR_ARG, "multinomial rows took left %d", sh.left);
  }
  CHECK(!torch_blob_ok(nullptr), "a null blob accepted");
}

// OptHelper::wake / OptCrew::Awake: the helper spins ahead of a call, runs nothing until the call posts, and goes back to sleep
// with or without a call in between.
void test_helper_wake() {
  OptCrew crew;
  { OptCrew::Awake a(crew); }                                  // no call follows
  for (int rep = 0; rep < 3; ++rep) {
    OptCrew::Awake a(crew);
    std::atomic<int> ran{0};
    crew.helper.begin([&] { ran.fetch_add(1); });              // what CrewCall's constructor does
    CHECK(ran.load() == 0, "the helper ran before it was asked");
    for (int i = 1; i <= 5; ++i) { crew.helper.wait(crew.helper.post()); CHECK(ran.load() == i, "round %d ran %d times", i, ran.load()); }
    crew.helper.end();
  }
  crew.shutdown();
}

// pcabo_sobol_draw_rows: ragged k, a skipped run, the boxes in pcabo_batch_acq_bounds' packing - equal to the per-run calls
void test_sobol_rows() {
  const int rows = 37, n = 130, kmax = 36;          // (more rows than a small batch)
  int ks[rows];
  for (int r = 0; r < rows; ++r) ks[r] = r == 0 ? 3 : r == 2 ? 1 : 1 + (r * 7) % 36;
  std::vector<std::vector<int64_t>> st(rows), sh(rows);
  std::vector<double> boxes((size_t)rows * 2 * kmax, NAN), out((size_t)rows * n * kmax, -7.0), one((size_t)n * kmax);
  std::vector<const int64_t*> sp(rows), hp(rows);
  std::vector<double*> op(rows);
  for (int r = 0; r < rows; ++r) {
    Lcg g(40 + r);
    st[r].resize((size_t)ks[r] * 30); sh[r].resize(ks[r]);
    for (auto& v : st[r]) v = (int64_t)(g.uni() * 1073741824.0);
    for (auto& v : sh[r]) v = (int64_t)(g.uni() * 1073741824.0);
    for (int j = 0; j < ks[r]; ++j) { boxes[(size_t)r * 2 * kmax + j] = -1.0 - j; boxes[(size_t)r * 2 * kmax + ks[r] + j] = 2.0 + r; }
    sp[r] = r == 2 ? nullptr : st[r].data(); hp[r] = sh[r].data(); op[r] = out.data() + (size_t)r * n * kmax;
  }
  CHECK(pcabo_sobol_draw_rows(sp.data(), hp.data(), ks, rows, n, boxes.data(), 2 * kmax, op.data()) == PCABO_OK, "draw rows");
  for (int r = 0; r < rows; ++r) {
    if (r == 2) { CHECK(op[r][0] == -7.0, "a skipped run was written"); continue; }
    std::vector<double> rng(ks[r]);
    for (int j = 0; j < ks[r]; ++j) rng[j] = boxes[(size_t)r * 2 * kmax + ks[r] + j] - boxes[(size_t)r * 2 * kmax + j];
    CHECK(pcabo_sobol_draw(st[r].data(), sh[r].data(), ks[r], n, boxes.data() + (size_t)r * 2 * kmax, rng.data(), one.data()) == PCABO_OK, "draw");
    for (int i = 0; i < n * ks[r]; ++i) CHECK(one[i] == op[r][i], "run %d element %d", r, i);
    if (ks[r] < kmax) CHECK(op[r][(size_t)n * ks[r]] == -7.0, "write behind the points of run %d", r);
  }
}

void test_plan() {
  std::vector<int> plan(LB_PLAN_INTS + 64, 0x5a5a5a5a);        // guard words behind the plan: they must stay
  for (int NP = 64; NP <= LB_MAXNP; NP += 64) {
    const int S = NP / 64;
    for (int n = NP - 63; n <= NP; ++n) {
      lb_build_plan_t(plan.data(), n, S);
      for (int i = LB_PLAN_INTS; i < (int)plan.size(); ++i) CHECK(plan[i] == 0x5a5a5a5a, "write behind the plan (n %d)", n);
      for (int pass = 0; pass < 2; ++pass) {
        const int* pw = plan.data() + pass * LB_PLAN_PASS;
        std::vector<int> cover(S * 512, 0);
        int max_dest = -1;
        for (int w = 0; w < LB_WAVES; ++w) {
          const int* e = pw + w * LB_PLAN_WAVE;
          CHECK(e[0] >= 0 && e[0] <= 2, "segments of a wave: %d", e[0]);
          for (int g = 0; g < e[0]; ++g) {
            const int u = e[1 + 4 * g], a = e[2 + 4 * g], b = e[3 + 4 * g], dest = e[4 + 4 * g];
            CHECK(u >= 0 && u < S && a >= 0 && b <= NP && a < b, "segment (%d, %d, %d)", u, a, b);
            CHECK(dest >= -1 && dest < lb_max_slots(NP), "slot %d of %d (n %d NP %d)", dest, lb_max_slots(NP), n, NP);
            if (dest > max_dest) max_dest = dest;
            for (int t = a; t < b && u >= 0 && u < S && t >= 0 && t < 512; ++t) cover[u * 512 + t] += 1;
          }
        }
        for (int u = 0; u < S; ++u) {
          const int lo = pass == 0 ? 0 : 64 * u, hi = pass == 0 ? (n < 64 * (u + 1) ? n : 64 * (u + 1)) : (n > 64 * u ? n : 64 * u);
          for (int t = 0; t < 512; ++t) CHECK(cover[u * 512 + t] == ((t >= lo && t < hi) ? 1 : 0), "pass %d unit %d index %d covered %d times (n %d)", pass, u, t, cover[u * 512 + t], n);
        }
      }
    }
  }
}

// One RestartGroup driven to its end on the CPU objective (each restart's point its own copy of the objective, the acquisition's
// signs: values -f, gradients -g); the points it evaluated, one after the other, into trail.
void drive_group(RestartGroup& rg, Objective& o, std::vector<double>* trail) {
  std::vector<double> hVal(rg.q0 + rg.nq), hGrad((size_t)(rg.q0 + rg.nq) * rg.k);
  while (rg.advance()) {
    if (trail) trail->insert(trail->end(), rg.x.begin(), rg.x.end());
    for (int j = 0; j < rg.nq; ++j) {
      double* gj = hGrad.data() + (size_t)(rg.q0 + j) * rg.k;
      hVal[rg.q0 + j] = -fg_objective(rg.x.data() + (size_t)j * rg.k, gj, &o);
      for (int c = 0; c < rg.k; ++c) gj[c] = -gj[c];
    }
    CHECK(rg.absorb(hVal.data(), hGrad.data(), rg.q0), "NaN gradient");
  }
}

// the joint problem of nq restarts: the sum of the restarts' objectives, in restart order
struct Joint { Objective* o; int nq, k; };
double fg_joint(const double* x, double* g, void* user) {
  const Joint* J = static_cast<const Joint*>(user);
  double f = 0.0;
  for (int j = 0; j < J->nq; ++j) f += fg_objective(x + (size_t)j * J->k, g + (size_t)j * J->k, J->o);
  return f;
}

void test_restart_group() {
  const int k = 9, nq = 4, q0 = 3, restarts = q0 + nq;
  Lcg r(31);
  Objective o; o.c.resize(k);
  for (auto& v : o.c) v = 2.0 * r.uni() - 1.0;
  std::vector<double> ics((size_t)restarts * k), bounds(2 * k);
  for (auto& v : ics) v = 4.0 * r.uni() - 2.0;
  for (int c = 0; c < k; ++c) { bounds[c] = -1.0 - 0.1 * c; bounds[k + c] = 1.25 + 0.05 * c; }
  // (a) the group is scipy's L-BFGS-B on the summed joint problem: negation and a sum in restart order are exact, so the
  // group and pcabo_lbfgsb_minimize take the same iterates and end on the same bits
  RestartGroup rg;
  rg.init(ics.data(), bounds.data(), q0, nq, k, 200);
  drive_group(rg, o, nullptr);
  std::vector<double> x(ics.begin() + (size_t)q0 * k, ics.end()), lo(nq * k), hi(nq * k);
  for (int t = 0; t < nq * k; ++t) { lo[t] = bounds[t % k]; hi[t] = bounds[k + t % k]; }
  Joint J{&o, nq, k};
  double f = 0.0; int nit = 0, nfev = 0, task = 0;
  const int wf = pcabo_lbfgsb_minimize(nq * k, x.data(), lo.data(), hi.data(), fg_joint, &J, 10, 1e7, 1e-5, 200, 15000, 20, &f, &nit, &nfev, &task);
  CHECK(std::memcmp(x.data(), rg.x.data(), x.size() * sizeof(double)) == 0, "group and joint minimize end on different points");
  CHECK(f == rg.f && nit == rg.niter && nfev == rg.nfev && wf == rg.opt.warnflag() && task == rg.opt.task(),
        "group f %.17g nit %d nfev %d, joint minimize f %.17g nit %d nfev %d", rg.f, rg.niter, rg.nfev, f, nit, nfev);
  CHECK(rg.niter > 2, "too short a run to compare: %d iterations", rg.niter);
  // (b) the order a group steps in is the one it was given: pcabo_lbfgsb_set_sum_order concerns pcabo_lbfgsb_minimize alone
  std::vector<double> trail0, trail1;
  RestartGroup g0, g1;
  g0.init(ics.data(), bounds.data(), q0, nq, k, 200, 0);
  drive_group(g0, o, &trail0);
  const int was = pcabo_lbfgsb_set_sum_order(1);
  g1.init(ics.data(), bounds.data(), q0, nq, k, 200, 0);
  drive_group(g1, o, &trail1);
  pcabo_lbfgsb_set_sum_order(was);
  CHECK(trail0.size() == trail1.size() && std::memcmp(trail0.data(), trail1.data(), trail0.size() * sizeof(double)) == 0,
        "a group of order 0 strays from its iterates while the process-wide order is 1 (%zu / %zu coordinates)",
        trail0.size(), trail1.size());
}

// ---- the single run's optimise call (OptCrew / CrewCall, pack_active / absorb_packed, free_pair of host_side.h) -------------------
// One call's inputs, and what a call leaves behind (the end points and values as the product takes them, the info rows)
struct OptProblem { int k, restarts, limit; Objective o; std::vector<double> ics, bounds; };
OptProblem opt_problem(int seed, int k, int restarts, int limit) {
  OptProblem P{k, restarts, limit, {}, {}, {}};
  Lcg r(seed);
  P.o.c.resize(k);
  for (auto& v : P.o.c) v = 2.0 * r.uni() - 1.0;
  P.ics.resize((size_t)restarts * k); P.bounds.resize(2 * k);
  for (auto& v : P.ics) v = 4.0 * r.uni() - 2.0;
  for (int c = 0; c < k; ++c) { P.bounds[c] = -1.0 - 0.1 * c; P.bounds[k + c] = 1.25 + 0.05 * c; }
  return P;
}
struct CallOut { std::vector<double> cand, vals; std::vector<int> info; };
CallOut call_out(RunRestarts& run, const OptProblem& P) {
  CallOut c{std::vector<double>((size_t)P.restarts * P.k, 0.0), std::vector<double>(P.restarts, 0.0), std::vector<int>(4 * run.grp.size(), 0)};
  run.end_points(c.cand.data(), c.vals.data());
  run.report(c.info.data(), 0);
  return c;
}
bool same_out(const CallOut& a, const CallOut& b) {
  return a.cand.size() == b.cand.size() && a.info == b.info && std::memcmp(a.cand.data(), b.cand.data(), a.cand.size() * sizeof(double)) == 0 &&
         std::memcmp(a.vals.data(), b.vals.data(), a.vals.size() * sizeof(double)) == 0;
}
// what the acquisition kernel would do with one query: the value -f and the gradient -g at x
void stub_query(const double* x, int k, Objective& o, double* val, double* grad) {
  *val = -fg_objective(x, grad, &o);
  for (int c = 0; c < k; ++c) grad[c] = -grad[c];
}
// The product's lock-step rounds until no group is active: advance all, pack, the stub evaluation of the packed points, absorb.
// trails[gi]: the points group gi was evaluated at.  Returns the number of rounds.
int lockstep_rounds(CrewCall& call, RunRestarts& run, const OptProblem& P, double* val, double* grad, std::vector<std::vector<double>>* trails) {
  std::vector<int> qoff(run.grp.size(), -1);
  Objective o = P.o;
  for (int rounds = 0;; ++rounds) {
    call.advance_all();
    const int nq = pack_active(run, qoff);
    if (nq == 0) return rounds;
    int expect = 0;
    for (size_t gi = 0; gi < run.grp.size(); ++gi) {
      const RestartGroup& rg = run.grp[gi];
      CHECK(qoff[gi] == (rg.active ? expect : -1), "group %zu packed at %d", gi, qoff[gi]);
      if (!rg.active) continue;
      CHECK(std::memcmp(run.xq + (size_t)qoff[gi] * P.k, rg.x.data(), rg.x.size() * sizeof(double)) == 0, "group %zu: packed point", gi);
      if (trails) (*trails)[gi].insert((*trails)[gi].end(), rg.x.begin(), rg.x.end());
      expect += rg.nq;
    }
    CHECK(expect == nq && nq <= P.restarts, "%d points packed, %d counted", nq, expect);
    for (int q = 0; q < nq; ++q) stub_query(run.xq + (size_t)q * P.k, P.k, o, val + q, grad + (size_t)q * P.k);
    CHECK(absorb_packed(run, qoff), "NaN gradient");
  }
}

// The stepping crew: for every number of threads the rule gives, a call's groups take the steps they take alone, byte for byte,
// whichever thread steps them; the helpers persist from call to call.
void test_crew() {
  OptCrew crew;
  const int counts[7] = {1, 2, 3, 11, 12, 16, 52}, threads[7] = {1, 2, 2, 2, 2, 3, 7};
  for (int ci = 0; ci < 7; ++ci) {
    const int ngroups = counts[ci], limit = 2;
    const OptProblem P = opt_problem(200 + ngroups, 4, limit * ngroups - 1, limit);       // the last group is short
    Objective o = P.o;
    std::vector<std::vector<double>> alone(ngroups);
    std::vector<RestartGroup> ref(ngroups);
    for (int gi = 0; gi < ngroups; ++gi) {
      ref[gi].init(P.ics.data(), P.bounds.data(), gi * limit, std::min(limit, P.restarts - gi * limit), P.k, 200);
      drive_group(ref[gi], o, &alone[gi]);
    }
    for (int call_no = 0; call_no < 2; ++call_no) {
      RunRestarts run;
      std::vector<double> xq((size_t)P.restarts * P.k), val(P.restarts), grad((size_t)P.restarts * P.k);
      run.init(P.ics.data(), P.bounds.data(), P.restarts, limit, P.k, 200);
      run.bind(xq.data(), val.data(), grad.data());
      std::vector<char> pending(ngroups, 0);
      std::vector<std::vector<double>> trails(ngroups);
      int rounds = 0;
      {
        CrewCall call(crew, run, pending);
        CHECK((int)run.grp.size() == ngroups && call.nh + 1 == threads[ci] && (ngroups == 1 || call.T == threads[ci]),
              "%d groups: %d helpers, T = %d", ngroups, call.nh, call.T);
        rounds = lockstep_rounds(call, run, P, val.data(), grad.data(), &trails);
      }
      int longest = 0;
      for (int gi = 0; gi < ngroups; ++gi) {
        const RestartGroup &a = run.grp[gi], &b = ref[gi];
        CHECK(trails[gi].size() == alone[gi].size() && std::memcmp(trails[gi].data(), alone[gi].data(), alone[gi].size() * sizeof(double)) == 0,
              "%d groups, call %d: group %d was evaluated at other points than alone", ngroups, call_no, gi);
        CHECK(a.niter == b.niter && a.nfev == b.nfev && a.opt.warnflag() == b.opt.warnflag() && a.opt.task() == b.opt.task() && !a.active,
              "%d groups, call %d: group %d: niter %d nfev %d, alone %d %d", ngroups, call_no, gi, a.niter, a.nfev, b.niter, b.nfev);
        CHECK(std::memcmp(a.x.data(), b.x.data(), b.x.size() * sizeof(double)) == 0, "%d groups: end point of group %d", ngroups, gi);
        longest = std::max(longest, (int)(alone[gi].size() / b.x.size()));
      }
      CHECK(rounds == longest && rounds > 2, "%d groups: %d rounds, the longest group took %d", ngroups, rounds, longest);
    }
  }
  CHECK(crew.more.size() == 5, "%zu further helpers", crew.more.size());
  crew.shutdown();
}

// The mailbox of free_pair in plain memory, and a thread in the place of the resident kernel.  ctl[q] = 2 tag + 1 (evaluate) or
// 2 tag (leave), release-stored behind the coordinates; the device answers query q by val[q], grad[q k ..] and then the tag,
// release-stored into pub[q].  Queries below `split` are group 0's.
struct StubMailbox {
  int cap, k, split;
  std::vector<double> x, val, grad;
  std::vector<std::atomic<unsigned long long>> ctl, pub;
  StubMailbox(int cap_, int k_, int split_) : cap(cap_), k(k_), split(split_), x((size_t)cap_ * k_), val(cap_), grad((size_t)cap_ * k_), ctl(cap_), pub(cap_) {
    for (int q = 0; q < cap; ++q) { ctl[q].store(0); pub[q].store(0); }
  }
  void post(int q0, int nq, const double* xs, unsigned long long tag) {
    std::memcpy(&x[(size_t)q0 * k], xs, (size_t)nq * k * sizeof(double));
    for (int j = 0; j < nq; ++j) ctl[q0 + j].store(2 * tag + 1, std::memory_order_release);
  }
  unsigned long long tag_of(int q) const { return pub[q].load(std::memory_order_acquire); }
  void leave(int q0, int nq, unsigned long long tag) { for (int j = 0; j < nq; ++j) ctl[q0 + j].store(2 * tag, std::memory_order_release); }
};
// How the stub device misbehaves.  mute: that group is never answered.  hold: that group gets no answer before the OTHER group
// has posted, then `free_rounds` answers (each `pace_us` late per query) and then none until the other group has left - so the
// held group is in the middle of its run, waiting or stepping, when the other group raises the abort flag, whichever thread
// the scheduler lets run first.  nan_q / nan_eval: that query's nan_eval-th answer carries a NaN gradient.
struct DeviceRules { int mute = -1, hold = -1, free_rounds = 0, pace_us = 0, nan_q = -1, nan_eval = 0; };
void stub_device(StubMailbox& mb, Objective o, DeviceRules R, std::vector<int>& evals) {
  std::vector<unsigned long long> seen(mb.cap, 0);
  std::vector<char> gone(mb.cap, 0);
  std::vector<int> after(mb.cap, 0);
  bool posted[2] = {false, false};
  int left[2] = {0, 0};
  const int size[2] = {mb.split, mb.cap - mb.split};
  while (left[0] + left[1] < mb.cap) {
    for (int q = 0; q < mb.cap; ++q) {
      if (gone[q]) continue;
      const unsigned long long c = mb.ctl[q].load(std::memory_order_acquire);
      if (c == seen[q]) continue;
      const int g = q >= mb.split ? 1 : 0;
      if (!(c & 1)) { seen[q] = c; gone[q] = 1; ++left[g]; continue; }
      posted[g] = true;
      if (g == R.mute) { seen[q] = c; continue; }
      if (g == R.hold) {                                                           // held: looked at again on the next sweep
        if (!posted[1 - g] || (after[q] >= R.free_rounds && left[1 - g] < size[1 - g])) continue;
        if (R.pace_us) std::this_thread::sleep_for(std::chrono::microseconds(R.pace_us));
        ++after[q];
      }
      seen[q] = c;
      stub_query(&mb.x[(size_t)q * mb.k], mb.k, o, &mb.val[q], &mb.grad[(size_t)q * mb.k]);
      if (++evals[q] == R.nan_eval && q == R.nan_q) mb.grad[(size_t)q * mb.k] = NAN;
      mb.pub[q].store(c >> 1, std::memory_order_release);
    }
    __builtin_ia32_pause();
  }
}

// The free-running pair: 7 restarts, limit 5 - two uneven groups, as the product's smallest such call.
void test_free_pair() {
  const OptProblem P = opt_problem(77, 3, 7, 5);
  const unsigned long long seq0 = 1000;
  OptCrew crew;
  // the pure lock-step call: what every variant below must end on
  CallOut want;
  int rounds_of[2] = {0, 0};
  {
    RunRestarts run;
    std::vector<double> xq((size_t)P.restarts * P.k), val(P.restarts), grad((size_t)P.restarts * P.k);
    run.init(P.ics.data(), P.bounds.data(), P.restarts, P.limit, P.k, 200);
    run.bind(xq.data(), val.data(), grad.data());
    std::vector<char> pending(2, 0);
    std::vector<std::vector<double>> trails(2);
    CrewCall call(crew, run, pending);
    lockstep_rounds(call, run, P, val.data(), grad.data(), &trails);
    want = call_out(run, P);
    for (int gi = 0; gi < 2; ++gi) rounds_of[gi] = (int)(trails[gi].size() / run.grp[gi].x.size());
    CHECK(rounds_of[0] > 10 && rounds_of[1] > 10, "too short runs to interrupt: %d and %d rounds", rounds_of[0], rounds_of[1]);
  }
  // One call: the first round in lock-step (as the product does before it knows that both groups are active), the pair on the
  // stub device under `rules`, then whatever the pair left in lock-step.
  struct PairRun { FreePair fp; char pending[2]; bool active[2]; std::vector<int> evals; CallOut out; int rounds_after; };
  const auto pair_call = [&](DeviceRules rules, std::chrono::nanoseconds timeout) {
    PairRun R;
    RunRestarts run;
    StubMailbox mb(P.restarts, P.k, P.limit);
    std::vector<double> xq((size_t)P.restarts * P.k);
    run.init(P.ics.data(), P.bounds.data(), P.restarts, P.limit, P.k, 200);
    run.bind(xq.data(), mb.val.data(), mb.grad.data());
    std::vector<char> pending(2, 0);
    std::vector<int> qoff(2, -1);
    R.evals.assign(P.restarts, 0);
    CrewCall call(crew, run, pending);
    call.advance_all();
    CHECK(pack_active(run, qoff) == P.restarts && qoff[0] == 0 && qoff[1] == P.limit, "both groups start active");
    std::thread device(stub_device, std::ref(mb), P.o, rules, std::ref(R.evals));
    R.fp = free_pair(call, run, mb, seq0, timeout);
    device.join();                                                           // (every query has been told to leave)
    for (int gi = 0; gi < 2; ++gi) { R.pending[gi] = pending[gi]; R.active[gi] = run.grp[gi].active; }
    R.rounds_after = 0;
    if (!R.fp.got_nan[0] && !R.fp.got_nan[1]) {
      R.rounds_after = lockstep_rounds(call, run, P, mb.val.data(), mb.grad.data(), nullptr);
      R.out = call_out(run, P);
    }
    return R;
  };
  // (a) both groups run to their stop, each on its own thread
  for (int rep = 0; rep < 2; ++rep) {
    const PairRun R = pair_call(DeviceRules(), std::chrono::seconds(3));
    for (int gi = 0; gi < 2; ++gi) {
      CHECK(!R.fp.timed_out[gi] && !R.fp.got_nan[gi] && !R.pending[gi] && !R.active[gi], "group %d did not run to its stop", gi);
      CHECK(R.fp.used[gi] == (unsigned long long)rounds_of[gi] + 1 && R.evals[gi * P.limit] == rounds_of[gi],
            "group %d used %llu tags and was answered %d times, %d rounds in lock-step", gi, R.fp.used[gi], R.evals[gi * P.limit], rounds_of[gi]);
    }
    CHECK(R.rounds_after == 0 && same_out(R.out, want), "the free pair ends elsewhere than the lock-step call");
  }
  // (b) group 1 is never answered: it times out and raises the abort flag; group 0, held in the middle of its run, sees it;
  // both wait for their evaluation and the lock-step rounds finish the call on the same bytes.  Which group's time-out comes
  // first must not hang on the scheduler of a busy machine: group 0's held round starts 4 rounds x 5 queries x 2 ms = 40 ms
  // after group 1 has posted, so it would time out 40 ms after group 1 - hence a time-out of 100 ms and not of a few.
  {
    DeviceRules rules;
    rules.mute = 1; rules.hold = 0; rules.free_rounds = 4; rules.pace_us = 2000;
    const PairRun R = pair_call(rules, std::chrono::milliseconds(100));
    CHECK(R.fp.timed_out[1] && !R.fp.timed_out[0] && !R.fp.got_nan[0] && !R.fp.got_nan[1], "time-outs %d %d", R.fp.timed_out[0], R.fp.timed_out[1]);
    CHECK(R.pending[0] == 1 && R.pending[1] == 1 && R.active[0] && R.active[1], "pending %d %d", R.pending[0], R.pending[1]);
    CHECK(R.fp.used[1] == 2 && R.fp.used[0] >= 2 && R.fp.used[0] < (unsigned long long)rounds_of[0] + 1, "tags used %llu %llu", R.fp.used[0], R.fp.used[1]);
    CHECK(R.evals[P.limit] == 0 && R.rounds_after > 0, "group 1 was answered %d times", R.evals[P.limit]);
    CHECK(same_out(R.out, want), "a call finished in lock-step after a time-out ends elsewhere than the lock-step call");
  }
  // (c) a NaN gradient in group 0's second answer: that group reports it, the other stops in the middle of its run
  {
    DeviceRules rules;
    rules.hold = 1; rules.free_rounds = 2; rules.nan_q = 0; rules.nan_eval = 2;
    const PairRun R = pair_call(rules, std::chrono::seconds(3));
    CHECK(R.fp.got_nan[0] && !R.fp.got_nan[1] && !R.fp.timed_out[0] && !R.fp.timed_out[1], "NaN flags %d %d", R.fp.got_nan[0], R.fp.got_nan[1]);
    CHECK(R.fp.used[0] == 3 && R.pending[1] == 1 && R.active[1] && R.fp.used[1] < (unsigned long long)rounds_of[1] + 1,
          "group 0 used %llu tags, group 1 %llu (pending %d)", R.fp.used[0], R.fp.used[1], R.pending[1]);
  }
  crew.shutdown();
}

// The product's round loop (run_rounds, host_side.h) over several "runs", stepped by the pool's workers: each worker drives its
// own runs with its own launch table on its stack; the stub evaluator does what the kernel would do with the table (the CPU
// objective, written into each run's host block).  Then the end points as the product takes them.
void test_gang_pool(int workers, int runs) {
  const int k = 7, nq = 5, ngroups = 2, restarts = nq * ngroups;
  std::vector<RunRestarts> run(runs);
  std::vector<Objective> obj(runs);
  std::vector<std::vector<double>> ics(runs), bounds(runs), hXq(runs), hVal(runs), hGrad(runs), cand(runs), vals(runs);
  for (int b = 0; b < runs; ++b) {
    Lcg r(100 + b);
    obj[b].c.resize(k);
    for (auto& v : obj[b].c) v = 2.0 * r.uni() - 1.0;
    ics[b].resize((size_t)restarts * k); bounds[b].resize(2 * k);
    for (auto& v : ics[b]) v = 4.0 * r.uni() - 2.0;
    for (int c = 0; c < k; ++c) { bounds[b][c] = -1.25; bounds[b][k + c] = 1.5; }
    hXq[b].assign((size_t)restarts * k, 0.0); hVal[b].assign(restarts, 0.0); hGrad[b].assign((size_t)restarts * k, 0.0);
    cand[b].assign((size_t)restarts * k, 0.0); vals[b].assign(restarts, 0.0);
    run[b].bind(hXq[b].data(), hVal[b].data(), hGrad[b].data());
  }
  GangPool pool;
  pool.start(workers);
  std::atomic<int> rounds{0};
  for (int call = 0; call < 3; ++call) {              // the pool is reused across calls, as a batch does per BO iteration
    // every second run steps in the device optimiser's order (the twin's setting)
    for (int b = 0; b < runs; ++b) run[b].init(ics[b].data(), bounds[b].data(), restarts, nq, k, 200, b & 1);
    pool.run([&](int t) {
      std::vector<int> mine;
      for (int b = t; b < runs; b += workers) mine.push_back(b);
      unsigned table[64];                              // the worker's own launch table
      int nent = 0;
      auto stage = [&](int b, const RestartGroup& rg) { if (nent < 64) table[nent++] = group_entry(b, rg.q0, rg.nq); };
      auto eval = [&] {                                // the stub evaluator: what the kernel would do with the table
        for (int e = 0; e < nent; ++e) {
          const int b = (int)(table[e] >> 16), q0 = (int)((table[e] >> 8) & 0xffu), cnt = (int)(table[e] & 0xffu);
          for (int j = 0; j < cnt; ++j) {
            double* g = hGrad[b].data() + (size_t)(q0 + j) * k;
            hVal[b][q0 + j] = -fg_objective(hXq[b].data() + (size_t)(q0 + j) * k, g, &obj[b]);
            for (int c = 0; c < k; ++c) g[c] = -g[c];  // (the acquisition is maximised: RestartGroup::absorb negates)
          }
        }
        nent = 0;
        rounds.fetch_add(1);
        return PCABO_OK;
      };
      CHECK(run_rounds(run.data(), mine, stage, eval) == PCABO_OK, "run_rounds failed");
      for (int b : mine) run[b].end_points(cand[b].data(), vals[b].data());
    });
    for (int b = 0; b < runs; ++b) {
      CHECK(run[b].status == PCABO_OK, "run %d: status %d", b, run[b].status);
      int info[4 * ngroups];
      run[b].report(info, 0);
      for (int gi = 0; gi < ngroups; ++gi) {
        const RestartGroup& rg = run[b].grp[gi];
        CHECK(!rg.active, "a group is still active after the call");
        CHECK(info[4 * gi] == rg.niter && info[4 * gi + 1] == rg.nfev && info[4 * gi + 2] == rg.opt.warnflag(), "report of group %d", gi);
        CHECK(rg.opt.warnflag() >= 0 && rg.opt.warnflag() <= 2, "warnflag");
        for (size_t i = 0; i < rg.x.size(); ++i) CHECK(rg.x[i] >= rg.lo[i] && rg.x[i] <= rg.hi[i], "end point outside the box");
        CHECK(std::memcmp(cand[b].data() + (size_t)rg.q0 * k, rg.x.data(), rg.x.size() * sizeof(double)) == 0, "end point of group %d", gi);
      }
    }
  }
  pool.shutdown();
  CHECK(rounds.load() > 0, "no rounds");
}

// ---- the GP hyperparameter fit (FitRun, fit_rounds, mll_assemble of host_side.h) over a stub evaluator --------------------------
// A small dense GP on the CPU: Matern-5/2 on the points as given, targets as given (the product's kernels normalise and
// standardise first; the stepper does not care), Cholesky and inverse by textbook loops.  th = {s2, c, rho} with one lengthscale,
// ard: {s2, c, rho_1 .. rho_k} with one per input.  h = the 5 + m sums the likelihood kernels hand to mll_assemble (m = 1, ard:
// m = k); false: K + s2 I is not positive definite.
struct TinyGP { int n = 0, k = 0; std::vector<double> Z, y; };
bool tiny_gp_sums(const TinyGP& gp, const double* th, double* h, bool ard = false) {
  const int n = gp.n, m = ard ? gp.k : 1;
  const double s2 = th[0], c = th[1], s5 = std::sqrt(5.0);
  const auto scaled = [&](int i, int j, int t) { return (gp.Z[i * gp.k + t] - gp.Z[j * gp.k + t]) / softplus_host(th[2 + (ard ? t : 0)]); };
  std::vector<double> K((size_t)n * n), G((size_t)n * n), L((size_t)n * n, 0.0), Li((size_t)n * n, 0.0), Kin((size_t)n * n), a(n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double r2 = 0.0;
      for (int t = 0; t < gp.k; ++t) { const double d = scaled(i, j, t); r2 += d * d; }
      const double r = std::sqrt(r2), e = std::exp(-s5 * r);
      K[i * n + j] = (1.0 + s5 * r + 5.0 / 3.0 * r2) * e + (i == j ? s2 : 0.0);
      G[i * n + j] = 5.0 / 3.0 * (1.0 + s5 * r) * e;                       // dK / dlog l_t = G d_t^2, dK / dlog l = G r^2
    }
  for (int j = 0; j < n; ++j)
    for (int i = j; i < n; ++i) {
      double v = K[i * n + j];
      for (int p = 0; p < j; ++p) v -= L[i * n + p] * L[j * n + p];
      if (i == j) { if (!(v > 0.0)) return false; L[j * n + j] = std::sqrt(v); }
      else L[i * n + j] = v / L[j * n + j];
    }
  for (int j = 0; j < n; ++j) {                                            // Li = L^-1, column by column
    Li[j * n + j] = 1.0 / L[j * n + j];
    for (int i = j + 1; i < n; ++i) {
      double v = 0.0;
      for (int p = j; p < i; ++p) v -= L[i * n + p] * Li[p * n + j];
      Li[i * n + j] = v / L[i * n + i];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {                                          // K^-1 = Li^T Li, alpha = K^-1 (y - c)
      double v = 0.0;
      for (int p = std::max(i, j); p < n; ++p) v += Li[p * n + i] * Li[p * n + j];
      Kin[i * n + j] = v;
      a[i] += v * (gp.y[j] - c);
    }
  for (int t = 0; t < 5 + m; ++t) h[t] = 0.0;
  for (int i = 0; i < n; ++i) {
    h[0] += std::log(L[i * n + i]); h[1] += (gp.y[i] - c) * a[i]; h[2] += a[i]; h[3] += a[i] * a[i]; h[4] += Kin[i * n + i];
    for (int j = 0; j < n; ++j)
      for (int t = 0; t < gp.k; ++t) {
        const double d = scaled(i, j, t);
        h[5 + (ard ? t : 0)] += (a[i] * a[j] - Kin[i * n + j]) * G[i * n + j] * (d * d);
      }
  }
  return true;
}
TinyGP tiny_gp(int seed, int n = 12, int k = 2) {
  Lcg r(seed);
  TinyGP gp; gp.n = n; gp.k = k; gp.Z.resize((size_t)n * k); gp.y.resize(n);
  for (auto& v : gp.Z) v = r.uni();
  for (int i = 0; i < n; ++i) gp.y[i] = std::sin(3.0 * gp.Z[i * k] + 0.3 * seed) + gp.Z[i * k + 1] * gp.Z[i * k + 1] - 0.6 + 0.1 * (r.uni() - 0.5);
  return gp;
}

// What a fit leaves behind, bit for bit
struct FitOut { int status; double theta[3], loss; int info[4]; };
FitOut fit_out(const FitRun& r) {
  FitOut o;
  std::memset(&o, 0, sizeof(o));
  o.status = r.status;
  if (r.status == PCABO_OK) { std::memcpy(o.theta, r.xr, sizeof(o.theta)); o.loss = r.fr; r.report(o.info); }
  return o;
}
const double FIT_START[3] = {0.006737946999085467, 0.0, 0.0};               // the model's initial values: (e^-5, 0, 0)

// The runs' fits over their GPs in lock-step (start[b] null: a parked run).  fail_at[b] > 0: run b's evaluation number fail_at[b]
// (1 = the start) answers PCABO_ERR_NOT_PD.  evals[b]: the thetas run b was evaluated at, the rounds it rested not counted;
// rested[b]: the rounds it rode along at its result.
struct FitDrive { std::vector<FitOut> out; std::vector<std::vector<double>> evals; std::vector<int> rested; int rounds = 0; };
FitDrive drive_fits(const std::vector<TinyGP>& gps, const std::vector<const double*>& start, const std::vector<int>& fail_at) {
  const size_t B = gps.size();
  std::vector<FitRun> runs(B);
  std::vector<double> hs(6 * B, 0.0);
  FitDrive d;
  d.evals.resize(B); d.rested.assign(B, 0);
  for (size_t b = 0; b < B; ++b) { runs[b].bind(&hs[6 * b]); if (start[b]) runs[b].init(start[b]); }
  const int rc = fit_rounds(runs, gps[0].n, [&](const std::vector<const double*>& th, int* st) {
    ++d.rounds;
    for (size_t b = 0; b < B; ++b) {
      const FitRun& r = runs[b];
      if (!th[b]) { CHECK(r.state == FitRun::OUT, "run %zu: no theta but not out", b); continue; }
      const bool resting = r.state == FitRun::RESTING;
      if (resting) {                                                         // rides along at its result
        CHECK(std::memcmp(th[b], r.xr, (size_t)r.nvar * sizeof(double)) == 0, "run %zu rests away from its result", b);
        ++d.rested[b];
      } else {
        d.evals[b].insert(d.evals[b].end(), th[b], th[b] + 3);
      }
      const bool fail = !resting && fail_at[b] > 0 && (int)d.evals[b].size() / 3 == fail_at[b];
      st[b] = !fail && tiny_gp_sums(gps[b], th[b], &hs[6 * b]) ? PCABO_OK : PCABO_ERR_NOT_PD;
    }
    return (int)PCABO_OK;
  });
  CHECK(rc == PCABO_OK, "fit_rounds: %d", rc);
  for (const FitRun& r : runs) {
    CHECK(r.state == FitRun::RESTING || r.state == FitRun::OUT, "a run is still stepping after the rounds");
    d.out.push_back(fit_out(r));
  }
  return d;
}

void test_fit_run() {
  // (0) mll_assemble's gradient belongs to its loss: central differences over the dense GP, step 1e-6 (times theta for s2).
  // Truncation ~ step^2 f''' / 6 and rounding ~ 1e-16 |f| / step both stay below 1e-8 here; the bound asked is 1e-6 (1 + |g|).
  {
    const TinyGP gp = tiny_gp(3);
    const double th[3] = {0.02, 0.15, -0.4};
    double h[6], f = 0.0, g[3], worst = 0.0;
    CHECK(tiny_gp_sums(gp, th, h), "the dense GP could not be factored");
    mll_assemble(h, gp.n, 1, th, &f, g);
    for (int i = 0; i < 3; ++i) {
      const double step = i == 0 ? 1e-6 * th[0] : 1e-6;
      double tp[3] = {th[0], th[1], th[2]}, tm[3] = {th[0], th[1], th[2]}, fp = 0.0, fm = 0.0;
      tp[i] += step; tm[i] -= step;
      CHECK(tiny_gp_sums(gp, tp, h), "factor"); mll_assemble(h, gp.n, 1, tp, &fp, nullptr);
      CHECK(tiny_gp_sums(gp, tm, h), "factor"); mll_assemble(h, gp.n, 1, tm, &fm, nullptr);
      const double fd = (fp - fm) / (tp[i] - tm[i]), err = std::fabs(fd - g[i]) / (1.0 + std::fabs(g[i]));
      if (err > worst) worst = err;
      CHECK(err < 1e-6, "gradient %d: %.12g against the difference quotient %.12g", i, g[i], fd);
    }
    std::printf("mll_assemble against central differences: worst %.2e (bound 1e-6)\n", worst);
  }
  // ... and in the ARD form, one rho per input (n = 8, k = 3; one rho above softplus's threshold, where the derivative is 1)
  {
    const TinyGP gp = tiny_gp(4, 8, 3);
    const int nv = 5;
    const double th[nv] = {0.03, -0.1, -0.4, 0.7, 20.5};
    double h[8], f = 0.0, g[nv], worst = 0.0;
    CHECK(mll_theta_ok(th, 3) && tiny_gp_sums(gp, th, h, true), "the dense ARD GP could not be factored");
    mll_assemble(h, gp.n, 3, th, &f, g);
    for (int i = 0; i < nv; ++i) {
      const double step = i == 0 ? 1e-6 * th[0] : 1e-6;
      double tp[nv], tm[nv], fp = 0.0, fm = 0.0;
      std::memcpy(tp, th, sizeof(th)); std::memcpy(tm, th, sizeof(th));
      tp[i] += step; tm[i] -= step;
      CHECK(tiny_gp_sums(gp, tp, h, true), "factor"); mll_assemble(h, gp.n, 3, tp, &fp, nullptr);
      CHECK(tiny_gp_sums(gp, tm, h, true), "factor"); mll_assemble(h, gp.n, 3, tm, &fm, nullptr);
      const double fd = (fp - fm) / (tp[i] - tm[i]), err = std::fabs(fd - g[i]) / (1.0 + std::fabs(g[i]));
      if (err > worst) worst = err;
      CHECK(err < 1e-6, "ARD gradient %d: %.12g against the difference quotient %.12g", i, g[i], fd);
    }
    std::printf("mll_assemble (ARD) against central differences: worst %.2e (bound 1e-6)\n", worst);
  }
  // ... and the shared lengthscale above the threshold: the loss takes ls = rho there, so the slope is 1, not the sigmoid
  // (1 - 1.25e-9 at 20.5, which the difference quotients above cannot tell from 1); at the threshold itself it is the sigmoid
  CHECK(softplus_slope(20.5) == 1.0, "the slope of softplus above the threshold is not 1");
  CHECK(softplus_slope(20.0) < 1.0 && softplus_slope(20.0) > 0.999999997, "the slope at the threshold is not the sigmoid");
  {
    const double th[3] = {0.05, 0.3, 20.5}, h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 2.0};
    double f = 0.0, g[3];
    mll_assemble(h, 4, 1, th, &f, g);
    CHECK(g[2] == -(0.5 * 2.0 * 1.0 / 20.5) / 4, "the shared lengthscale's gradient at rho = 20.5 is not -S / (2 rho n)");
  }
  // (a) B runs in lock-step = every run alone: theta, loss, info bit for bit; finished runs ride along at their result and are
  // not counted
  const int B = 5;
  std::vector<TinyGP> gps;
  for (int b = 0; b < B; ++b) gps.push_back(tiny_gp(10 + b));
  const FitDrive all = drive_fits(gps, std::vector<const double*>(B, FIT_START), std::vector<int>(B, 0));
  int rested = 0, nfev_min = 1 << 30, nfev_max = 0;
  for (int b = 0; b < B; ++b) {
    const FitDrive one = drive_fits({gps[b]}, {FIT_START}, {0});
    CHECK(all.out[b].status == PCABO_OK && all.out[b].info[0] > 2, "run %d: status %d after %d iterations", b, all.out[b].status, all.out[b].info[0]);
    CHECK(std::memcmp(&all.out[b], &one.out[0], sizeof(FitOut)) == 0, "run %d in lock-step differs from the run alone", b);
    CHECK(all.evals[b] == one.evals[0], "run %d was evaluated at other points in lock-step", b);
    CHECK(all.out[b].info[1] <= (int)all.evals[b].size() / 3, "run %d counts %d evaluations of %zu", b, all.out[b].info[1], all.evals[b].size() / 3);
    CHECK(one.rested[0] == 0 && one.rounds == (int)one.evals[0].size() / 3, "a run alone took a round without an evaluation");
    rested += all.rested[b];
    nfev_min = std::min(nfev_min, all.out[b].info[1]); nfev_max = std::max(nfev_max, all.out[b].info[1]);
  }
  CHECK(nfev_min < nfev_max && rested > 0, "no run finished before another (evaluations %d .. %d): nothing rode along", nfev_min, nfev_max);
  {                                                        // a parked run (never started) stays out and is never evaluated
    const FitDrive d = drive_fits({gps[0], gps[1]}, {nullptr, FIT_START}, {0, 0});
    CHECK(d.out[0].status == PCABO_ERR_ARG && d.evals[0].empty(), "a parked run was stepped");
    CHECK(std::memcmp(&d.out[1], &all.out[1], sizeof(FitOut)) == 0, "a run beside a parked run differs from the run alone");
  }
  // (b) PCABO_ERR_NOT_PD at evaluation e of run 0, for every e, run 1 beside it undisturbed: the fit stops at the last accepted
  // iterate (warnflag 2, task NOT_PD) and asks for one more evaluation THERE - also when that iterate was the last point
  // evaluated (the failing trial was the first of its line search).  At e = 1 (the start) the run fails.
  const int total = (int)all.evals[0].size() / 3;
  int end_at_last_evaluated = 0;
  for (int e = 1; e <= total; ++e) {
    const FitDrive d = drive_fits({gps[0], gps[1]}, {FIT_START, FIT_START}, {e, 0});
    CHECK(std::memcmp(&d.out[1], &all.out[1], sizeof(FitOut)) == 0, "failure %d of run 0 disturbed run 1", e);
    const FitOut& o = d.out[0];
    const std::vector<double>& ev = d.evals[0];
    if (e == 1) { CHECK(o.status == PCABO_ERR_NOT_PD && ev.size() == 3, "start not factored: status %d", o.status); continue; }
    CHECK(o.status == PCABO_OK && o.info[2] == 2 && o.info[3] == PCABO_FIT_TASK_NOT_PD, "failure %d: status %d warnflag %d task %d", e, o.status, o.info[2], o.info[3]);
    CHECK(o.info[1] == e - 1, "failure %d: %d evaluations counted", e, o.info[1]);
    CHECK((int)ev.size() / 3 == e + 1 && std::memcmp(&ev[3 * e], o.theta, sizeof(o.theta)) == 0, "failure %d: no evaluation at the result behind it", e);
    bool evaluated = false;                                // the result is a point the run had evaluated
    for (int i = 0; i < e - 1; ++i) evaluated = evaluated || std::memcmp(&ev[3 * i], o.theta, sizeof(o.theta)) == 0;
    CHECK(evaluated, "failure %d: the result was never evaluated", e);
    if (std::memcmp(&ev[3 * (e - 2)], o.theta, sizeof(o.theta)) == 0) ++end_at_last_evaluated;
    double h[6], f = 0.0;
    CHECK(tiny_gp_sums(gps[0], o.theta, h), "factor"); mll_assemble(h, gps[0].n, 1, o.theta, &f, nullptr);
    CHECK(f == o.loss, "failure %d: the loss is not the one at the result", e);
  }
  CHECK(end_at_last_evaluated > 0, "no failure met the first trial of a line search");
  // (c) a trial theta outside the model's domain.  The sums of a loss that falls linearly in rho (slope G, no pull on s2 and c):
  // after the first iteration the line search keeps extrapolating (rho = -1, -3, -11, ... -683) until softplus(rho) underflows to
  // 0 - the fit stops at the last accepted iterate, task DOMAIN, and is evaluated once more there.  A start out there is the run's
  // error, PCABO_ERR_ARG, and nothing is evaluated.
  {
    std::vector<FitRun> run(1);
    double h[6] = {0, 0, 0, 0, 0, 0};
    int evals = 0;
    std::vector<double> rhos;
    const int n = 12;
    const double G = 0.5;
    const auto linear = [&](const std::vector<const double*>& th, int* st) {
      const double s2 = th[0][0], rho = th[0][2], u = std::log(s2) + 4.0;
      CHECK(mll_theta_ok(th[0], 1), "asked to evaluate a theta outside the domain");
      h[1] = 2.0 * n * G * rho; h[5] = -2.0 * n * G * softplus_host(rho) * (1.0 + std::exp(-rho)); h[3] = 2.0 * (1.0 + u) / s2;
      ++evals; rhos.push_back(rho); st[0] = PCABO_OK;
      return (int)PCABO_OK;
    };
    run[0].bind(h); run[0].init(FIT_START);
    CHECK(fit_rounds(run, n, linear) == PCABO_OK, "fit_rounds");
    const FitOut o = fit_out(run[0]);
    CHECK(o.status == PCABO_OK && o.info[2] == 2 && o.info[3] == PCABO_FIT_TASK_DOMAIN, "domain stop: status %d warnflag %d task %d", o.status, o.info[2], o.info[3]);
    CHECK(o.info[0] >= 1 && evals == o.info[1] + 1 && evals > 3, "domain stop: %d iterations, %d evaluations, %d counted", o.info[0], evals, o.info[1]);
    CHECK(rhos.back() == o.theta[2] && rhos[evals - 2] < -600.0 && std::count(rhos.begin(), rhos.end(), o.theta[2]) == 2,
          "domain stop: the result rho %g is not an earlier iterate evaluated again at the end (last trial %g)", o.theta[2], rhos[evals - 2]);
    const double far[3] = {FIT_START[0], 0.0, -800.0};
    evals = 0;
    run[0].init(far);
    CHECK(fit_rounds(run, n, linear) == PCABO_OK, "fit_rounds");
    CHECK(run[0].status == PCABO_ERR_ARG && run[0].state == FitRun::OUT && evals == 0, "start outside the domain: status %d, %d evaluations", run[0].status, evals);
  }
  // (d) a shared-lengthscale run and an ARD run (k = 3, one start below the bound on rho_c: clipped to it) in one vector: each
  // takes the fit it takes alone, bit for bit, and the ARD run keeps every rho_c at or above its bound
  {
    const TinyGP gp2[2] = {tiny_gp(10), tiny_gp(5, 12, 3)};
    const double start_ard[5] = {FIT_START[0], 0.0, 0.0, -100.0, 0.0};
    struct Out { int status, nvar, info[4]; double theta[5], loss; };
    const auto drive = [&](const std::vector<int>& which) {
      std::vector<FitRun> runs(which.size());
      std::vector<double> hs(8 * which.size(), 0.0);
      for (size_t b = 0; b < which.size(); ++b) {
        runs[b].bind(&hs[8 * b]);
        if (which[b]) runs[b].init(start_ard, 3, true); else runs[b].init(FIT_START);
      }
      CHECK(fit_rounds(runs, 12, [&](const std::vector<const double*>& th, int* st) {
        for (size_t b = 0; b < which.size(); ++b)
          if (th[b]) st[b] = tiny_gp_sums(gp2[which[b]], th[b], &hs[8 * b], which[b] != 0) ? PCABO_OK : PCABO_ERR_NOT_PD;
        return (int)PCABO_OK;
      }) == PCABO_OK, "fit_rounds");
      std::vector<Out> out(which.size());
      for (size_t b = 0; b < which.size(); ++b) {
        Out& o = out[b];
        std::memset(&o, 0, sizeof(o));
        o.status = runs[b].status; o.nvar = runs[b].nvar;
        CHECK(o.status == PCABO_OK && o.nvar == (which[b] ? 5 : 3), "run %zu: status %d, %d variables", b, o.status, o.nvar);
        if (o.status != PCABO_OK) continue;
        std::memcpy(o.theta, runs[b].xr, (size_t)o.nvar * sizeof(double)); o.loss = runs[b].fr; runs[b].report(o.info);
      }
      return out;
    };
    const std::vector<Out> both = drive({0, 1}), swapped = drive({1, 0});
    for (int f = 0; f < 2; ++f) {
      const std::vector<Out> one = drive({f});
      CHECK(std::memcmp(&both[f], &one[0], sizeof(Out)) == 0 && std::memcmp(&swapped[1 - f], &one[0], sizeof(Out)) == 0,
            "the %s run beside the other form differs from the run alone", f ? "ARD" : "shared-lengthscale");
      CHECK(one[0].info[0] > 2 && one[0].info[1] > one[0].info[0], "form %d: %d iterations, %d evaluations", f, one[0].info[0], one[0].info[1]);
    }
    for (int j = 2; j < 5; ++j) CHECK(both[1].theta[j] >= FIT_ARD_RHO_MIN, "rho_%d = %g below its bound", j - 2, both[1].theta[j]);
    CHECK(both[0].info[1] != both[1].info[1], "the two runs finished in the same round: neither rode along");
  }
  // (e) the batch's ARD round (pcabo_batch_gp_fit_ard): B ARD runs of different m = k_b (3, 1, 2, 4) stepped side by side, their
  // sums at a common stride (5 + the largest m, as the strided copy of the results leaves them), one run parked (never started,
  // never evaluated: it rides along at the shared model).  Every run takes the fit it takes alone, bit for bit; the runs do not all
  // finish in the same round.
  {
    const int ks[4] = {3, 1, 2, 4}, KMAX = 4, HS = 5 + KMAX, B4 = 4;
    std::vector<TinyGP> gps4;
    for (int b = 0; b < B4; ++b) gps4.push_back(tiny_gp(20 + b, 12, std::max(ks[b], 2)));   // (tiny_gp's target reads two inputs)
    for (int b = 0; b < B4; ++b)
      if (ks[b] < gps4[b].k) {                             // keep the first ks[b] inputs only
        TinyGP g; g.n = gps4[b].n; g.k = ks[b]; g.y = gps4[b].y; g.Z.resize((size_t)g.n * g.k);
        for (int i = 0; i < g.n; ++i) for (int t = 0; t < g.k; ++t) g.Z[i * g.k + t] = gps4[b].Z[i * gps4[b].k + t];
        gps4[b] = g;
      }
    struct Out { int status, nvar, info[4]; double theta[2 + 4], loss; };
    const auto drive = [&](const std::vector<int>& which, int parked) {
      const size_t nb = which.size();
      std::vector<FitRun> runs(nb);
      std::vector<double> hs((size_t)HS * nb, 0.0);
      std::vector<int> evals(nb, 0);
      for (size_t b = 0; b < nb; ++b) {
        double start[2 + 4] = {FIT_START[0], 0.0, 0.0, 0.0, 0.0, 0.0};
        runs[b].bind(&hs[(size_t)HS * b]);
        if ((int)b != parked) runs[b].init(start, gps4[which[b]].k, true);
      }
      int rounds = 0;
      CHECK(fit_rounds(runs, 12, [&](const std::vector<const double*>& th, int* st) {
        ++rounds;
        for (size_t b = 0; b < nb; ++b) {
          if (!th[b]) { CHECK(runs[b].state == FitRun::OUT, "run %zu: no theta but not out", b); continue; }
          CHECK((int)b != parked, "the parked run was evaluated");
          if (runs[b].state != FitRun::RESTING) ++evals[b];
          st[b] = tiny_gp_sums(gps4[which[b]], th[b], &hs[(size_t)HS * b], true) ? PCABO_OK : PCABO_ERR_NOT_PD;
        }
        return (int)PCABO_OK;
      }) == PCABO_OK, "fit_rounds");
      std::vector<Out> out(nb);
      for (size_t b = 0; b < nb; ++b) {
        Out& o = out[b];
        std::memset(&o, 0, sizeof(o));
        o.status = runs[b].status; o.nvar = runs[b].nvar;
        if (o.status != PCABO_OK) continue;
        CHECK(o.nvar == 2 + gps4[which[b]].k, "run %zu: %d variables", b, o.nvar);
        std::memcpy(o.theta, runs[b].xr, (size_t)o.nvar * sizeof(double)); o.loss = runs[b].fr; runs[b].report(o.info);
        CHECK(evals[b] >= o.info[1] && rounds >= evals[b], "run %zu: %d evaluations counted, %d made, %d rounds", b, o.info[1], evals[b], rounds);
      }
      return out;
    };
    const std::vector<Out> all4 = drive({0, 1, 2, 3}, -1), parked4 = drive({0, 1, 2, 3}, 1);
    int emin = 1 << 30, emax = 0;
    for (int b = 0; b < B4; ++b) {
      const std::vector<Out> one = drive({b}, -1);
      CHECK(one[0].status == PCABO_OK && one[0].info[0] > 2, "ARD run %d alone: status %d after %d iterations", b, one[0].status, one[0].info[0]);
      CHECK(std::memcmp(&all4[b], &one[0], sizeof(Out)) == 0, "ARD run %d (m = %d) in lock-step differs from the run alone", b, ks[b]);
      if (b == 1) CHECK(parked4[b].status == PCABO_ERR_ARG, "the parked ARD run has status %d", parked4[b].status);
      else CHECK(std::memcmp(&parked4[b], &one[0], sizeof(Out)) == 0, "ARD run %d beside a parked run differs from the run alone", b);
      emin = std::min(emin, one[0].info[1]); emax = std::max(emax, one[0].info[1]);
    }
    CHECK(emin < emax, "the ARD runs all took %d evaluations: nothing rode along", emin);
  }
}

// The host's inverse map (host_side.h) against the loop of k_inverse_map written out coordinate by coordinate: one fused
// multiply-add per term, c ascending, then the two means.  Bytes equal, for both forms of the chain, at the edges of the kernel's
// 8-way unroll and with exact and signed zeros; one case whose result differs between a fused and an unfused multiply-add.
void test_inverse_map_host() {
  const auto reference = [](const double* z, const double* comps, const double* pm, const double* dm, int k, int d, double* x) {
    for (int j = 0; j < d; ++j) {
      double s = 0.0;
      for (int c = 0; c < k; ++c) s = std::fma(z[c], comps[(size_t)c * d + j], s);
      x[j] = (s + pm[j]) + dm[j];
    }
  };
  for (int k : {1, 7, 8, 9, 36, 40})
    for (int d : {1, 40, 100}) {
      Lcg r(1000 * k + d);
      std::vector<double> z(k), comps((size_t)k * d), pm(d), dm(d), x(d), xs(d), xr(d);
      for (int rep = 0; rep < 51; ++rep) {
        for (auto& v : z) v = 2e3 * r.uni() - 1e3;
        for (auto& v : comps) v = 2.0 * r.uni() - 1.0;
        for (auto& v : pm) v = 2.0 * r.uni() - 1.0;
        for (auto& v : dm) v = 10.0 * r.uni() - 5.0;
        if (rep == 50) {                                   // exact zeros and signed zeros
          for (int c = 0; c < k; ++c) z[c] = (c & 1) ? -0.0 : 0.0;
          for (size_t i = 0; i < comps.size(); i += 3) comps[i] = (i & 1) ? -0.0 : 0.0;
          for (int j = 0; j < d; ++j) { pm[j] = (j & 1) ? -0.0 : 0.0; dm[j] = (j & 2) ? -0.0 : 0.0; }
        }
        reference(z.data(), comps.data(), pm.data(), dm.data(), k, d, xr.data());
        inverse_map_host(z.data(), comps.data(), pm.data(), dm.data(), k, d, x.data());
        inverse_map_host(z.data(), comps.data(), pm.data(), dm.data(), k, d, xs.data(), false);
        CHECK(std::memcmp(x.data(), xr.data(), d * sizeof(double)) == 0, "inverse map k %d d %d rep %d: not the fused chain's bits", k, d, rep);
        CHECK(std::memcmp(xs.data(), xr.data(), d * sizeof(double)) == 0, "inverse map k %d d %d rep %d: std::fma form differs", k, d, rep);
      }
    }
  const double e30 = std::ldexp(1.0, -30), z[2] = {-(1.0 + 2.0 * e30), 1.0 + e30}, comps[2] = {1.0, 1.0 + e30}, zero = 0.0;
  double x = -1.0;
  inverse_map_host(z, comps, &zero, &zero, 2, 1, &x);
  CHECK(x == std::ldexp(1.0, -60), "inverse map: the chain is not fused (got %g, an unfused product gives 0)", x);
}

// The layout of a context's memory (ctx_layout.h), arithmetic only: no region is allocated, no pointer formed.  For every shape of
// the sweep: the buffers in carving order, apart, 256-byte aligned, the regions multiples of 4096 bytes and two calls alike (what
// lets a batch address every run with one stride); every secondary use of a buffer inside its landlord at its largest legal
// arguments, and the uses that are live together apart; the fitting predicates against the inequalities they replaced, written out
// here once as they stood at the call sites.  For four shapes every offset and both region sizes against a recorded table: the
// numbers were printed by the hand-written carving code that ctx_layout() replaced, not by ctx_layout() itself, so a change of an
// offset fails here (the batched kernels' single stride and the bit-pinned tests rest on the layout).
void test_ctx_layout() {
  struct Pinned { int shape[3]; size_t dev_bytes, host_bytes, dev[D_COUNT], host[H_COUNT]; };
  static const Pinned pinned[] = {
    {{2, 1, 1}, 262144, 12288,
    {
     0, 256, 512, 768, 1024, 1792, 2048, 2304, 2560, 4608, 4864, 5120, 5376, 5632, 5888, 6144, 6400, 6656, 7168, 7424, 11520,
     12544, 14592, 16640, 18688, 19200, 51968, 84736, 117504, 118016, 118528, 184064, 184320, 192768, 193024, 193280, 193536,
     193792, 194048, 194560, 260096, 260352, 261376},
    {
     0, 4608, 8192, 8448, 8704, 9472, 9728, 9984, 10240, 11264}},
    {{90, 5, 16}, 876544, 24576,
    {
     0, 3840, 7680, 8448, 9216, 21248, 22016, 22528, 31232, 33280, 33536, 33792, 34048, 37888, 38144, 38400, 38656, 39424,
     40448, 40704, 44800, 45824, 47872, 56064, 64256, 65280, 196352, 327424, 458496, 459520, 460544, 526080, 526848, 791040,
     791296, 792064, 792320, 792576, 792832, 809216, 874752, 875264, 876288},
    {
     0, 4608, 8192, 8448, 9216, 10496, 19200, 19456, 19712, 20736}},
    {{450, 40, 512}, 44011520, 651264,
    {
     0, 144128, 288256, 292096, 295936, 470272, 474112, 487936, 783360, 801792, 814592, 827392, 827904, 972032, 972288, 972544,
     972800, 976640, 980736, 980992, 985088, 986112, 988160, 1152000, 1315840, 1319936, 3417088, 5514240, 7611392, 7615488,
     7619584, 7685120, 7849216, 41665792, 41669888, 41833728, 41834240, 41834752, 41835008, 43932160, 43997696, 44009984,
     44011008},
    {
     0, 4608, 168704, 172800, 336640, 352512, 647936, 648192, 648704, 649728}},
    {{513, 128, 64}, 18243584, 1339392,
    {
     0, 525312, 1050624, 1054976, 1059328, 1588736, 1593088, 1727232, 2786304, 2917376, 3048448, 3179520, 3180544, 3705856,
     3706112, 3706368, 3706624, 3710976, 3715584, 3715840, 3719936, 3720960, 3723008, 4312832, 4902656, 4907264, 7561472,
     10215680, 12869888, 12874496, 12879104, 12944640, 13010432, 17765888, 17766400, 17831936, 17832960, 17833984, 17834240,
     18129152, 18194688, 18242304, 18243328},
    {
     0, 4608, 70400, 70912, 136448, 276224, 1335296, 1335552, 1336832, 1337856}},
  };
  for (const Pinned& p : pinned) {
    const CtxLayout L = ctx_layout(ctx_shape(p.shape[0], p.shape[1], p.shape[2]));
    CHECK(L.dev_bytes == p.dev_bytes && L.host_bytes == p.host_bytes, "layout (%d, %d, %d): region sizes %zu / %zu", p.shape[0], p.shape[1], p.shape[2], L.dev_bytes, L.host_bytes);
    for (int i = 0; i < D_COUNT; ++i) CHECK(L.dev[i].off == p.dev[i], "layout (%d, %d, %d): device buffer %d at %zu, recorded %zu", p.shape[0], p.shape[1], p.shape[2], i, L.dev[i].off, p.dev[i]);
    for (int i = 0; i < H_COUNT; ++i) CHECK(L.host[i].off == p.host[i], "layout (%d, %d, %d): host buffer %d at %zu, recorded %zu", p.shape[0], p.shape[1], p.shape[2], i, L.host[i].off, p.host[i]);
  }
  const auto region_ok = [](const Buf* b, int count, size_t bytes) {
    size_t end = 0;
    for (int i = 0; i < count; ++i) {
      if (b[i].off % 256 != 0 || b[i].off < end || b[i].count == 0 || b[i].elem == 0) return false;
      end = b[i].off + b[i].count * b[i].elem;
    }
    return bytes % 4096 == 0 && end <= bytes && bytes - end < 4096;
  };
  const int ns[] = {2, 63, 64, 65, 448, 512, 513, 1280, 4096}, ds[] = {1, 3, 4, 5, 16, 17, 40, 41, 128};
  const int qs[] = {1, 15, 16, 32, 63, 64, 72, 512, PCABO_CNT_DONE - 1};
  CHECK(!ctx_sizes_ok(1, 1, 1) && !ctx_sizes_ok(2, 0, 1) && !ctx_sizes_ok(2, PCABO_MAXD + 1, 1) && !ctx_sizes_ok(2, 1, 0) &&
        !ctx_sizes_ok(2, 1, PCABO_CNT_DONE), "ctx_sizes_ok lets a shape beyond the limits through");
  for (int max_n : ns) for (int max_d : ds) for (int max_q : qs) {
    CHECK(ctx_sizes_ok(max_n, max_d, max_q), "shape (%d, %d, %d) refused", max_n, max_d, max_q);
    const CtxShape s = ctx_shape(max_n, max_d, max_q);
    const CtxLayout L = ctx_layout(s), L2 = ctx_layout(ctx_shape(max_n, max_d, max_q));
#define LCHECK(c, what) CHECK(c, "layout (%d, %d, %d): %s", max_n, max_d, max_q, what)
    LCHECK(s.NPcap % PCABO_BS == 0 && s.NPcap >= max_n && s.NPcap - max_n < PCABO_BS && s.DPcap % 16 == 0 && s.DPcap >= max_d &&
           s.KPcap % 4 == 0 && s.KPcap >= max_d && s.KPcap - max_d < 4 && s.Scap * PCABO_SLAB == s.NPcap, "the padded capacities");
    LCHECK(region_ok(L.dev, D_COUNT, L.dev_bytes), "device buffers out of order, overlapping or unaligned");
    LCHECK(region_ok(L.host, H_COUNT, L.host_bytes), "host buffers out of order, overlapping or unaligned");
    LCHECK(std::memcmp(L.dev, L2.dev, sizeof(L.dev)) == 0 && std::memcmp(L.host, L2.host, sizeof(L.host)) == 0 &&
           L.dev_bytes == L2.dev_bytes && L.host_bytes == L2.host_bytes, "two calls disagree");
    const Buf &partial = L.dev[D_PARTIAL], &xq = L.dev[D_XQ], &hxq = L.host[H_XQ], &small = L.host[H_SMALL];
    // dPartial: the extend scratch, the leave-one-out block, the posterior's records and results
    LCHECK(fits(partial_ext_scratch(s), partial), "the extend scratch");
    LCHECK(fits(partial_loo(max_n), partial) && partial_loo_part(max_n, 3) + max_n == partial_loo(max_n).count, "the leave-one-out block");
    for (int q : {1, max_q}) for (int NP : {64, s.NPcap}) {
      const Use rec = partial_post_records(q, NP), res = partial_post_result(q, NP);
      LCHECK(fits(rec, partial) && fits(res, partial) && apart(rec, res), "the posterior's records and results");
    }
    // dXq: the extend's rows and values; rows_cap as the call site had it
    LCHECK(fits(xq_queries(s), xq) && fits(xq_queries(s), hxq) && xq_queries(s).count + PCABO_XQ_TAIL == xq.count, "the query block");
    for (int k = 1; k <= max_d; ++k) {
      const int rows_cap = ext_rows_cap(s, k);
      const Use rows = xq_ext_rows(s, k), vals = xq_ext_vals(s, k);
      LCHECK(rows_cap >= 1 && rows_cap == (int)(((size_t)max_q * max_d + 8) / ((size_t)k + 1)), "rows_cap");
      LCHECK((size_t)rows_cap * (k + 1) <= xq.count && fits(rows, xq) && fits(vals, xq) && apart(rows, vals), "the extend's rows and values");
    }
    // the device optimiser: opt_fits against `max_q < 64 + 8 ngroups || (num_restarts + 2) kmax > max_q max_d`, and its tenants
    for (int nr : {1, 5, 10, 32}) for (int bl : {1, 5}) for (int kmax : {1, max_d}) {
      const int ngroups = opt_groups(nr, bl);
      const bool was = !(max_q < 64 + 8 * ngroups || (size_t)(nr + 2) * kmax > (size_t)max_q * max_d);
      LCHECK(ngroups == (nr + bl - 1) / bl && opt_fits(L, nr, ngroups, kmax) == was, "the device optimiser's eligibility");
      // (its evaluation-only entry point asked `max_q < 64` alone)
      LCHECK(opt_fits(L, nr, 0, kmax) == !(max_q < 64), "the device evaluation's eligibility");
      if (!was) continue;
      const Use pts = xq_opt_points(nr, kmax), cands = grad_opt_cands(nr, kmax), vals = val_opt_values(nr), rec = val_opt_records(ngroups);
      LCHECK(fits(pts, xq) && fits(pts, hxq), "the device optimiser's points");
      LCHECK(fits(cands, L.dev[D_GRAD]) && fits(cands, L.host[H_GRAD]), "the device optimiser's candidates");
      LCHECK(fits(vals, L.dev[D_VAL]) && fits(rec, L.dev[D_VAL]) && fits(rec, L.host[H_VAL]) && apart(vals, rec) &&
             val_opt_record(0) == 64 && val_opt_record(ngroups - 1) + 8 == rec.start + rec.count, "the device optimiser's values and records");
    }
    // the fit's results behind the widest run's tile partials, on both sides
    for (int M : {1, s.KPcap}) {
      const Use part = mll_partials(s.NPcap, M), res = mll_result(s.NPcap, M);
      LCHECK(fits(part, L.dev[D_MLL]) && fits(res, L.dev[D_MLL]) && apart(part, res) && fits(hmll_result(M), L.host[H_MLL]) &&
             hmll_result(M).count == res.count, "the fit's results");
    }
    // hSmall at k = d = max_d: the wPCA results, the inverse map's x, a batch's Normalize bounds
    const Use w = small_wpca(s), x = small_imap_x(s), nb = small_norm_bounds(s);
    const PcaParts pp = pca_parts(s);
    LCHECK(fits(w, small) && fits(x, small) && fits(nb, small) && apart(w, x) && apart(w, nb) && apart(x, nb), "the three tenants of hSmall");
    LCHECK(x.count >= (size_t)max_d && nb.count >= 2 * (size_t)max_d && pca_copy_count(s, max_d, max_d) == w.count && w.count == L.dev[D_PCAOUT].count &&
           pp.data_mean + max_d <= pp.pca_mean && pp.pca_mean + max_d <= pp.evr && pp.evr + max_d <= pp.comps, "the wPCA result block");
    // the packed inputs, the tickets, the transposed root inverse, the kernel vectors' rows
    LCHECK(in_pack(max_n, max_d, true, true, true).total == L.dev[D_IN].count && L.dev[D_IN].count == L.host[H_IN].count, "the packed inputs");
    LCHECK(fits(counters_queries(max_q), L.dev[D_COUNTERS]) && fits(counters_group(), L.dev[D_COUNTERS]) &&
           apart(counters_queries(PCABO_QFLAG_WORDS), counters_group()), "the tickets");
    LCHECK(fits(gram_rt(s.NPcap, s.NPcap), L.dev[D_GRAM]), "the transposed root inverse");
#undef LCHECK
  }
}

// The call state (model_state.h): a record is driven through the legal call sequences of a BO iteration, for a context and for a
// batch with three member runs, and after every step EVERY field is compared with values written out here - what the assignment
// sites of pcabo_api.hip left before the record existed - and every question with a table that restates the call-order rules of
// include/pcabo.h.  The slab count is the launcher's (acq_slabs: NP / 16 at these sizes), handed in as pcabo_api.hip hands it in.
struct MS {      // a ModelState written out, in the order of its declaration
  int n, n_base, d, k, KP, NP; double ls, s2; int kernel; double rung;
  bool have_wpca, unc; int wn, wd; bool pending, have_gp, zn, rt; int cnt_S; bool dirty; int gcur, vprev_d;
};
void expect_state(const ModelState& s, const MS& e, const char* what) {
  CHECK(s.n == e.n && s.n_base == e.n_base && s.d == e.d && s.k == e.k && s.KP == e.KP && s.NP == e.NP,
        "%s: shape n %d n_base %d d %d k %d KP %d NP %d", what, s.n, s.n_base, s.d, s.k, s.KP, s.NP);
  CHECK(s.lengthscale == e.ls && s.noise == e.s2 && s.kernel == e.kernel && s.rung == e.rung,
        "%s: hyperparameters %g %g %d rung %g", what, s.lengthscale, s.noise, s.kernel, s.rung);
  CHECK(s.have_wpca == e.have_wpca && s.wpca_uncollected == e.unc && s.wpca_n == e.wn && s.wpca_d == e.wd,
        "%s: wPCA phase %d %d (%d x %d)", what, s.have_wpca, s.wpca_uncollected, s.wpca_n, s.wpca_d);
  CHECK(s.gp_pending == e.pending && s.have_gp == e.have_gp && s.zn_recorded == e.zn && s.rt_stale == e.rt,
        "%s: GP phase pending %d have_gp %d zn %d rt_stale %d", what, s.gp_pending, s.have_gp, s.zn_recorded, s.rt_stale);
  CHECK(s.cnt_S == e.cnt_S && s.cnt_dirty == e.dirty && s.gcur == e.gcur && s.vprev_d == e.vprev_d,
        "%s: tickets %d %d, ping-pong %d %d", what, s.cnt_S, s.cnt_dirty, s.gcur, s.vprev_d);
}
// the questions of a context's entry points: pcabo_wpca / _begin refuse while in flight, pcabo_gp_condition_end(_eval) need one in
// flight, the calls on the conditioned model need GP_READY, Z == NULL needs the wPCA of these very (n, k), and the tickets
struct MQ { bool in_flight; GpReady ready; bool wpca_known, z_null_3_1, z_null_64_5, reset_4, reset_8; };
void expect_answers(const ModelState& s, const MQ& e, const char* what) {
  CHECK(s.in_flight() == e.in_flight && s.gp_ready() == e.ready && s.conditioned() == (e.ready == GP_READY) && s.wpca_known() == e.wpca_known, "%s: in flight %d ready %d wPCA known %d",
        what, s.in_flight(), (int)s.gp_ready(), s.wpca_known());
  CHECK(s.wpca_matches(3, 1) == e.z_null_3_1 && s.wpca_matches(64, 5) == e.z_null_64_5 && !s.wpca_matches(3, 2) && !s.wpca_matches(65, 1),
        "%s: Z == NULL allowed for (3, 1): %d, (64, 5): %d", what, s.wpca_matches(3, 1), s.wpca_matches(64, 5));
  CHECK(s.tickets_need_reset(4) == e.reset_4 && s.tickets_need_reset(8) == e.reset_8, "%s: tickets need a reset for 4 slabs %d, 8 slabs %d",
        what, s.tickets_need_reset(4), s.tickets_need_reset(8));
}

void test_model_state() {
  const auto slabs = [](int NP) { return NP / 16; };
  const double LS = 0.75, S2 = 1e-3; const int KN = PCABO_KERNEL_MATERN52;
  const bool T = true, F = false;
  {  // ---- a context ----
    ModelState s;
    expect_state(s, {0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0.0, F, F, 0, 0, F, F, F, F, 0, T, 0, 0}, "a new context");
    expect_answers(s, {F, GP_NONE, F, F, F, T, T}, "a new context");
    // pcabo_wpca (n = 3, d = 2, k = 1), then pcabo_gp_condition_begin with k known, pcabo_gp_condition_end on rung 0
    CHECK(!s.warm_start(2), "no eigenvectors to start from yet");
    s.wpca_enqueued(3, 2); s.points_replaced(3);
    expect_state(s, {3, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0.0, F, F, 3, 2, F, F, F, F, 0, T, 1, 2}, "wPCA enqueued");
    expect_answers(s, {F, GP_NONE, F, F, F, T, T}, "wPCA enqueued");
    s.wpca_collected(1);
    expect_state(s, {3, 0, 2, 1, 4, 0, 0.0, 0.0, 0, 0.0, T, F, 3, 2, F, F, F, F, 0, T, 1, 2}, "wPCA collected");
    expect_answers(s, {F, GP_NONE, T, T, F, T, T}, "wPCA collected");
    s.condition_enqueued(3, 1, LS, S2, KN, true);
    CHECK(s.tickets_reset_if_needed(slabs(s.NP)), "the first conditioning resets the tickets");
    expect_state(s, {3, 3, 2, 1, 4, 64, LS, S2, KN, 0.0, T, F, 3, 2, T, F, T, F, 4, F, 1, 2}, "conditioning enqueued (k known)");
    expect_answers(s, {T, GP_IN_FLIGHT, T, T, F, F, T}, "conditioning enqueued (k known)");
    s.condition_ended_ok(0.0);
    expect_state(s, {3, 3, 2, 1, 4, 64, LS, S2, KN, 0.0, T, F, 3, 2, F, T, T, F, 4, F, 1, 2}, "conditioning ended on rung 0");
    expect_answers(s, {F, GP_READY, T, T, F, F, T}, "conditioning ended on rung 0");
    // pcabo_wpca_gp_condition_begin (n = 64, k on the device), pcabo_wpca_results (k = 5), pcabo_gp_condition_end_eval on 1e-7
    CHECK(s.warm_start(2) && !s.warm_start(3), "the previous eigenvectors serve a wPCA of the same d only");
    s.wpca_enqueued(64, 2);
    s.condition_enqueued(64, -1, LS, S2, KN, true);
    CHECK(!s.tickets_reset_if_needed(slabs(s.NP)), "n = 64 has the slab count of n = 3: no reset");
    expect_state(s, {64, 64, 2, 1, 4, 64, LS, S2, KN, 0.0, T, T, 64, 2, T, F, T, F, 4, F, 0, 2}, "conditioning enqueued (k on the device)");
    expect_answers(s, {T, GP_IN_FLIGHT, T, F, F, F, T}, "conditioning enqueued (k on the device)");
    s.wpca_collected(5);
    expect_state(s, {64, 64, 2, 5, 8, 64, LS, S2, KN, 0.0, T, F, 64, 2, T, F, T, F, 4, F, 0, 2}, "wPCA results behind the conditioning");
    expect_answers(s, {T, GP_IN_FLIGHT, T, F, T, F, T}, "wPCA results behind the conditioning");
    ModelState failed = s, plain = s;
    CHECK(s.zn_consumed() && !s.zn_consumed(), "the event behind k_znorm is taken once");
    s.condition_ended_ok(1e-7);                        // (the jitter redo of pcabo_gp_condition_end_eval ends through pcabo_gp_condition_end)
    expect_state(s, {64, 64, 2, 5, 8, 64, LS, S2, KN, 1e-7, T, F, 64, 2, F, T, F, F, 4, F, 0, 2}, "conditioning ended on rung 1e-7");
    expect_answers(s, {F, GP_READY, T, F, T, F, T}, "conditioning ended on rung 1e-7");
    failed.condition_failed();
    expect_state(failed, {64, 64, 2, 5, 8, 64, LS, S2, KN, 0.0, T, F, 64, 2, F, F, T, F, 4, F, 0, 2}, "conditioning failed");
    expect_answers(failed, {F, GP_NONE, T, F, T, F, T}, "conditioning failed");
    (void)plain.zn_consumed(); plain.condition_ended_ok(0.0);      // pcabo_gp_condition_end_eval without a redo
    expect_state(plain, {64, 64, 2, 5, 8, 64, LS, S2, KN, 0.0, T, F, 64, 2, F, T, F, F, 4, F, 0, 2}, "end_eval without a jitter redo");
    expect_answers(plain, {F, GP_READY, T, F, T, F, T}, "end_eval without a jitter redo");
    // one evaluation of a fit (pcabo_gp_mll): the conditioning at theta, ended inside the call
    s.condition_enqueued(64, 5, 1.0, 0.02, KN, true);
    CHECK(!s.tickets_reset_if_needed(slabs(s.NP)), "a fit evaluation at the same n: no reset");
    s.condition_ended_ok(1e-8);
    expect_state(s, {64, 64, 2, 5, 8, 64, 1.0, 0.02, KN, 1e-8, T, F, 64, 2, F, T, T, F, 4, F, 0, 2}, "fit evaluation");
    expect_answers(s, {F, GP_READY, T, F, T, F, T}, "fit evaluation");
    // pcabo_get_gram, then the device optimiser's rebuild; the option switched on behind a conditioning
    s.gram_fetched();
    expect_state(s, {64, 64, 2, 5, 8, 64, 1.0, 0.02, KN, 1e-8, T, F, 64, 2, F, T, T, T, 4, F, 0, 2}, "Gram fetched");
    expect_answers(s, {F, GP_READY, T, F, T, F, T}, "Gram fetched");
    s.rt_rebuilt(); CHECK(!s.rt_stale, "rebuilt: fresh");
    s.rt_wanted(); CHECK(s.rt_stale, "the device optimiser switched on behind a conditioning: stale");
    s.rt_rebuilt(); failed.rt_wanted(); CHECK(!failed.rt_stale, "no GP: nothing to rebuild");
    // pcabo_gp_extend across NP (64 -> 65) and pcabo_gp_truncate back: n_base held, the tickets follow the slab count
    s.n_changed(65);
    CHECK(s.tickets_reset_if_needed(slabs(s.NP)), "65 points: 8 slab groups, the tickets are reset");
    expect_state(s, {65, 64, 2, 5, 8, 128, 1.0, 0.02, KN, 1e-8, T, F, 64, 2, F, T, T, T, 8, F, 0, 2}, "extended to 65");
    expect_answers(s, {F, GP_READY, T, F, F, T, F}, "extended to 65");
    s.n_changed(64);
    CHECK(s.tickets_reset_if_needed(slabs(s.NP)), "back to 64 points: 4 slab groups again");
    expect_state(s, {64, 64, 2, 5, 8, 64, 1.0, 0.02, KN, 1e-8, T, F, 64, 2, F, T, T, T, 4, F, 0, 2}, "truncated to 64");
    expect_answers(s, {F, GP_READY, T, F, T, F, T}, "truncated to 64");
    // a second conditioning with another n; a launch that may have died
    s.wpca_enqueued(65, 2);
    s.condition_enqueued(65, -1, LS, S2, KN, false);
    CHECK(s.tickets_reset_if_needed(slabs(s.NP)), "conditioning at n = 65: reset");
    expect_state(s, {65, 65, 2, 5, 8, 128, LS, S2, KN, 0.0, T, T, 65, 2, T, F, F, T, 8, F, 1, 2}, "second conditioning");
    expect_answers(s, {T, GP_IN_FLIGHT, T, F, F, T, F}, "second conditioning");
    s.launch_may_have_died();
    expect_answers(s, {T, GP_IN_FLIGHT, T, F, F, T, T}, "a launch may have died: a reset is due at the same slab count");
    CHECK(s.tickets_reset_if_needed(8) && !s.tickets_need_reset(8) && !s.cnt_dirty, "the reset clears the mark");
  }
  {  // ---- a batch of three runs: k = 1, 5, 5; run 1 fails its factorisation, run 2 ends on a jitter rung ----
    BatchState b;
    ModelState r[3];
    const std::vector<ModelState*> runs = {&r[0], &r[1], &r[2]};
    const int ks[3] = {1, 5, 5};
    const auto expect_batch = [&](const MS& e, bool fitted, bool score, bool imap, bool opt, GpReady ready, bool scorable, bool on_host, const char* what) {
      expect_state(b.m, e, what);
      CHECK(b.fitted == fitted && b.score_enqueued == score && b.imap_enqueued == imap && b.opt_enqueued == opt, "%s: pending halves", what);
      CHECK(b.begin_pending() == (score || imap || opt) && b.gp_ready() == ready && b.scorable() == scorable && b.wpca_on_host() == on_host &&
            b.anything_enqueued() == (e.n != 0 || e.unc), "%s: the batch's answers", what);
    };
    expect_batch({0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0.0, F, F, 0, 0, F, F, F, F, 0, T, 0, 0}, F, F, F, F, GP_NONE, F, F, "a new batch");
    // pcabo_batch_wpca_gp_condition_begin, n = 3, d = 2
    b.m.wpca_enqueued(3, 2);
    CHECK(b.tickets_reset_if_needed(slabs(64), runs), "the first conditioning resets every run's tickets");
    b.condition_enqueued(3, 2, -1, LS, S2, KN);
    for (int i = 0; i < 3; ++i) r[i].follow(b, r[i].own().with_k(r[i].k).started(LS, S2));
    expect_batch({3, 3, 2, 0, 0, 64, LS, S2, KN, 0.0, F, T, 3, 2, T, F, F, F, 4, F, 1, 2}, F, F, F, F, GP_IN_FLIGHT, T, F, "batch conditioning enqueued");
    for (int i = 0; i < 3; ++i)      // (a member has nothing in flight of its own: single-context calls on it are refused for want of a GP)
      expect_state(r[i], {3, 3, 2, 0, 0, 64, LS, S2, KN, 0.0, F, F, 0, 0, F, F, F, F, 4, F, 1, 2}, "a member behind the batch's conditioning");
    for (int i = 0; i < 3; ++i) expect_answers(r[i], {F, GP_NONE, F, F, F, F, T}, "a member behind the batch's conditioning");
    // pcabo_batch_wpca_results
    b.wpca_collected();
    for (int i = 0; i < 3; ++i) r[i].follow(b, r[i].own().with_k(ks[i]));
    expect_batch({3, 3, 2, 0, 0, 64, LS, S2, KN, 0.0, T, F, 3, 2, T, F, F, F, 4, F, 1, 2}, F, F, F, F, GP_IN_FLIGHT, T, T, "batch wPCA collected");
    expect_state(r[0], {3, 3, 2, 1, 4, 64, LS, S2, KN, 0.0, T, F, 0, 0, F, F, F, F, 4, F, 1, 2}, "member 0 behind the wPCA results");
    expect_state(r[2], {3, 3, 2, 5, 8, 64, LS, S2, KN, 0.0, T, F, 0, 0, F, F, F, F, 4, F, 1, 2}, "member 2 behind the wPCA results");
    expect_answers(r[0], {F, GP_NONE, T, T, F, F, T}, "member 0 behind the wPCA results");
    expect_answers(r[2], {F, GP_NONE, T, F, F, F, T}, "member 2 behind the wPCA results");
    // pcabo_batch_gp_condition_end_eval_begin / _end: run 1's ladder fails, run 2's ends on 1e-7 (their own records are told)
    b.scoring_begun();
    expect_batch({3, 3, 2, 0, 0, 64, LS, S2, KN, 0.0, T, F, 3, 2, T, F, F, F, 4, F, 1, 2}, F, T, F, F, GP_IN_FLIGHT, T, T, "scoring enqueued");
    b.scoring_ended();
    r[1].condition_failed(); r[2].condition_ended_ok(1e-7);
    const bool ok[3] = {T, F, T};
    for (int i = 0; i < 3; ++i) r[i].follow(b, r[i].own().ended(ok[i]));
    expect_batch({3, 3, 2, 0, 0, 64, LS, S2, KN, 0.0, T, F, 3, 2, F, T, F, F, 4, F, 1, 2}, F, F, F, F, GP_READY, F, T, "scoring collected");
    expect_state(r[0], {3, 3, 2, 1, 4, 64, LS, S2, KN, 0.0, T, F, 0, 0, F, T, F, F, 4, F, 1, 2}, "member 0 conditioned");
    expect_state(r[1], {3, 3, 2, 5, 8, 64, LS, S2, KN, 0.0, T, F, 0, 0, F, F, F, F, 4, F, 1, 2}, "member 1 without a GP");
    expect_state(r[2], {3, 3, 2, 5, 8, 64, LS, S2, KN, 1e-7, T, F, 0, 0, F, T, F, F, 4, F, 1, 2}, "member 2 on rung 1e-7");
    expect_answers(r[0], {F, GP_READY, T, T, F, F, T}, "member 0 conditioned");
    expect_answers(r[1], {F, GP_NONE, T, F, F, F, T}, "member 1 without a GP");
    expect_answers(r[2], {F, GP_READY, T, F, F, F, T}, "member 2 on rung 1e-7");
    // the other pending halves
    b.opt_begun(8, 4);
    CHECK(b.opt_matches(8, 4) && !b.opt_matches(8, 5) && !b.opt_matches(7, 4) && b.gp_ready() == GP_IN_FLIGHT && b.begin_pending(), "optimisation enqueued");
    b.opt_ended();
    CHECK(!b.opt_matches(8, 4) && b.gp_ready() == GP_READY, "optimisation collected");
    b.imap_begun(); CHECK(b.imap_enqueued && b.gp_ready() == GP_IN_FLIGHT, "inverse map enqueued");
    b.imap_ended(); CHECK(!b.begin_pending() && b.gp_ready() == GP_READY, "inverse map collected");
    // a second conditioning at n = 64 and a lock-step fit behind it: a round starts every run at its own hyperparameters
    b.m.wpca_enqueued(64, 2);
    CHECK(!b.tickets_reset_if_needed(slabs(64), runs), "same slab count, nobody dirty: no reset");
    b.condition_enqueued(64, 2, -1, LS, S2, KN);
    for (int i = 0; i < 3; ++i) r[i].follow(b, r[i].own().with_k(r[i].k).started(LS, S2));
    b.wpca_collected();
    for (int i = 0; i < 3; ++i) r[i].follow(b, r[i].own().with_k(ks[i]));
    expect_state(r[2], {64, 64, 2, 5, 8, 64, LS, S2, KN, 0.0, T, F, 0, 0, F, F, F, F, 4, F, 0, 2}, "member 2 behind the second conditioning");
    expect_answers(r[2], {F, GP_NONE, T, F, T, F, T}, "member 2 behind the second conditioning");
    const double ls_own[3] = {0.5, LS, 1.0}, s2_own[3] = {0.01, S2, 0.02};      // (run 1 is parked: it rests at the shared model)
    for (int i = 0; i < 3; ++i) r[i].follow(b, r[i].own().started(ls_own[i], s2_own[i]));
    expect_state(r[0], {64, 64, 2, 1, 4, 64, 0.5, 0.01, KN, 0.0, T, F, 0, 0, F, F, F, F, 4, F, 0, 2}, "member 0 in a fit round");
    expect_answers(r[0], {F, GP_NONE, T, F, F, F, T}, "member 0 in a fit round");
    r[2].condition_ended_ok(1e-8);                     // its round failed: redone alone on its own context
    r[0].follow(b, r[0].own().ended(true)); r[1].follow(b, r[1].own().ended(true));
    b.fit_finished();
    r[1].follow(b, r[1].own().ended(false));           // (pcabo_batch_gp_fit: a run whose fit failed is left without a GP)
    expect_batch({64, 64, 2, 0, 0, 64, LS, S2, KN, 0.0, T, F, 64, 2, F, T, F, F, 4, F, 0, 2}, T, F, F, F, GP_READY, T, T, "fit finished");
    expect_state(r[0], {64, 64, 2, 1, 4, 64, 0.5, 0.01, KN, 0.0, T, F, 0, 0, F, T, F, F, 4, F, 0, 2}, "member 0 fitted");
    expect_state(r[1], {64, 64, 2, 5, 8, 64, LS, S2, KN, 0.0, T, F, 0, 0, F, F, F, F, 4, F, 0, 2}, "member 1 after a failed fit");
    expect_state(r[2], {64, 64, 2, 5, 8, 64, 1.0, 0.02, KN, 1e-8, T, F, 0, 0, F, T, F, F, 4, F, 0, 2}, "member 2 fitted on rung 1e-8");
    expect_answers(r[0], {F, GP_READY, T, F, F, F, T}, "member 0 fitted");
    expect_answers(r[1], {F, GP_NONE, T, F, T, F, T}, "member 1 after a failed fit");
    expect_answers(r[2], {F, GP_READY, T, F, T, F, T}, "member 2 fitted on rung 1e-8");
    for (int i = 0; i < 3; ++i) r[i].follow(b, r[i].own().with_k(ks[i]));      // pcabo_batch_wpca_results once more: the fitted models stay
    expect_state(r[0], {64, 64, 2, 1, 4, 64, 0.5, 0.01, KN, 0.0, T, F, 0, 0, F, T, F, F, 4, F, 0, 2}, "member 0 keeps its fitted model");
    expect_answers(r[0], {F, GP_READY, T, F, F, F, T}, "member 0 keeps its fitted model");
    // pcabo_batch_gp_condition_begin (no wPCA: k = d = 5 for every run) at n = 65: the fit is over, the tickets follow NP
    CHECK(b.tickets_reset_if_needed(slabs(128), runs), "65 points: reset");
    b.condition_enqueued(65, 5, 5, LS, S2, KN);
    for (int i = 0; i < 3; ++i) { r[i].rt_rebuilt(); r[i].follow(b, r[i].own().with_k(5).started(LS, S2)); }
    expect_batch({65, 65, 5, 5, 8, 128, LS, S2, KN, 0.0, F, F, 64, 2, T, F, F, F, 8, F, 0, 2}, F, F, F, F, GP_IN_FLIGHT, T, T, "conditioning without a wPCA");
    expect_state(r[0], {65, 65, 5, 5, 8, 128, LS, S2, KN, 0.0, F, F, 0, 0, F, F, F, F, 8, F, 0, 2}, "member 0 behind it");
    expect_answers(r[0], {F, GP_NONE, F, F, F, T, F}, "member 0 behind the conditioning without a wPCA");
    {  // (a conditioning without a wPCA clears a batch's uncollected mark; one with it sets it)
      BatchState c2 = b; c2.m.wpca_enqueued(65, 5); c2.condition_enqueued(65, 5, -1, LS, S2, KN);
      CHECK(c2.m.wpca_uncollected && !c2.wpca_on_host(), "k on the device: the wPCA is uncollected");
      c2.condition_enqueued(65, 5, 5, LS, S2, KN);
      CHECK(!c2.m.wpca_uncollected && c2.wpca_on_host(), "k known: no wPCA goes with the conditioning");
    }
    // dirty tickets: a single-context call on member 1 timed out
    r[1].launch_may_have_died();
    CHECK(b.tickets_need_reset(8, runs) && !b.m.tickets_need_reset(8), "a member's mark makes the batch's reset due at an unchanged NP");
    r[1].follow(b, r[1].own().ended(true));
    CHECK(r[1].cnt_dirty && b.tickets_need_reset(8, runs), "following the batch does not clear a member's mark");
    CHECK(b.tickets_reset_if_needed(8, runs), "the next conditioning resets");
    CHECK(!b.m.cnt_dirty && !r[0].cnt_dirty && !r[1].cnt_dirty && !r[2].cnt_dirty && r[1].cnt_S == 8, "the reset clears the mark on the batch and on every member");
    CHECK(!b.tickets_need_reset(8, runs) && b.tickets_need_reset(4, runs), "no mark, same slab count: no reset");
    // the transposed root inverse: Gram fetched -> stale, the conditioning's rebuild -> fresh, extend -> stale
    r[0].condition_ended_ok(0.0);
    r[0].gram_fetched(); CHECK(r[0].rt_stale, "Gram fetched: stale");
    r[0].rt_rebuilt(); CHECK(!r[0].rt_stale, "the conditioning's rebuild: fresh");
    r[0].n_changed(66); CHECK(r[0].rt_stale && r[0].n_base == 65, "extend: stale, n_base held");
  }
}

}  // namespace

int main(int argc, char** argv) {
  const int workers = argc > 1 ? std::atoi(argv[1]) : 4;
  test_minimize();
  test_sobol();
  test_sobol_rows();
  test_torch_rng();
  test_helper_wake();
  test_plan();
  test_restart_group();
  test_crew();
  test_free_pair();
  test_fit_run();
  test_inverse_map_host();
  test_ctx_layout();
  test_model_state();
  test_gang_pool(1, 3);
  test_gang_pool(workers, 11);
  if (g_fail) { std::fprintf(stderr, "host selftest: %d check(s) failed\n", g_fail); return 1; }
  std::printf("host selftest ok\n");
  return 0;
}
