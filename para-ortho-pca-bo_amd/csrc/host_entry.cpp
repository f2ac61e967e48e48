// Entry points of include/pcabo.h that are host code only (no HIP call, no device): the L-BFGS-B driver the tests pin against
// scipy, the switch of its vector kernels and the Sobol helpers (torch.quasirandom.SobolEngine restated; reference call site:
// botorch's gen_batch_initial_conditions behind /root/reference/Algorithms/BayesianOptimization/PCA_BO.py:607-614).
// Built by g++ into libpcabo.so and, with -fsanitize=..., into the host-only checker libraries of the Makefile.
#include "../../include/pcabo.h"
#include "host_side.h"
#include "lbfgsb.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" {

namespace {
std::atomic<int> g_minimize_sum_order{0};                     // pcabo_lbfgsb_set_sum_order: read by pcabo_lbfgsb_minimize alone
thread_local unsigned g_last_branches[LBB_COUNT] = {};        // the branch counters of this thread's last pcabo_lbfgsb_minimize
}

int pcabo_lbfgsb_minimize(int nvar, double* x, const double* lower, const double* upper, pcabo_fg_callback fg,
                          void* user, int m, double factr, double pgtol, int maxiter, int maxfun, int maxls,
                          double* f_out, int* nit, int* nfev, int* task_out) {
  if (nvar < 1 || !x || !fg || m < 1) return PCABO_ERR_ARG;
  LbfgsbDriver run;
  run.init(nvar, x, lower, upper, g_minimize_sum_order.load(), maxiter, maxfun, m, factr, pgtol, maxls);
  while (run.advance()) run.absorb(fg(run.x.data(), run.g.data(), user));
  std::copy(run.x.begin(), run.x.end(), x);
  if (f_out) *f_out = run.f;
  if (nit) *nit = run.niter;
  if (nfev) *nfev = run.nfev;
  if (task_out) *task_out = run.opt.task();
  { std::vector<double> end((size_t)nvar); run.end_point(end.data()); }      // (counted only: botorch's end, as the restart groups take it)
  std::copy(run.opt.branches(), run.opt.branches() + LBB_COUNT, g_last_branches);
  return run.opt.warnflag();
}

// Debug exports, not part of the ABI in include/pcabo.h (tests/test_lbfgsb_branches_cpu.py).  The names of the optimiser's branch
// counters (lbfgsb.h), comma-separated, into buf; returns their number.
int pcabo_debug_lbfgsb_branch_names(char* buf, int cap) {
  if (buf && cap > 0) {
    size_t at = 0;
    buf[0] = 0;
    for (int i = 0; i < LBB_COUNT; ++i) {
      const char* nm = lbfgsb_branch_name(i);
      const size_t len = strlen(nm);
      if (at + len + 2 > (size_t)cap) break;
      if (i) buf[at++] = ',';
      memcpy(buf + at, nm, len + 1);
      at += len;
    }
  }
  return LBB_COUNT;
}
// The counters of the calling thread's last pcabo_lbfgsb_minimize into out[0 .. min(cap, LBB_COUNT)); returns LBB_COUNT.
int pcabo_debug_lbfgsb_branches(unsigned* out, int cap) {
  if (out) for (int i = 0; i < LBB_COUNT && i < cap; ++i) out[i] = g_last_branches[i];
  return LBB_COUNT;
}

int pcabo_lbfgsb_set_vector_kernels(int enabled) { return lbfgsb_set_vector_kernels(enabled); }
int pcabo_lbfgsb_set_sum_order(int order) { return g_minimize_sum_order.exchange(order ? 1 : 0); }

int pcabo_sobol_scramble(int64_t* state, const int64_t* ltm, int k) {
  if (!state || !ltm || k < 1) return PCABO_ERR_ARG;
  const int MAXBIT = 30;
  for (int d = 0; d < k; ++d) {
    // matrix d over GF(2): unit diagonal, entries below it from ltm, nothing above (whatever ltm holds there - the caller
    // need not clear the upper triangle).  col[c] = column c as a bit vector, row p at bit MAXBIT-1-p.
    int64_t col[30];
    for (int c = 0; c < MAXBIT; ++c) col[c] = (int64_t)1 << (MAXBIT - 1 - c);
    for (int p = 1; p < MAXBIT; ++p) {
      const int64_t* row = ltm + ((size_t)d * MAXBIT + p) * MAXBIT;
      const int64_t pbit = (int64_t)1 << (MAXBIT - 1 - p);
      for (int c = 0; c < p; ++c) col[c] |= (row[c] & 1) ? pbit : 0;
    }
    for (int j = 0; j < MAXBIT; ++j) {                  // state <- matrix * state, bit MAXBIT-1-c of the state = component c
      unsigned long long v = (unsigned long long)state[(size_t)d * MAXBIT + j] & ((1ull << MAXBIT) - 1);
      int64_t t2 = 0;
      while (v) {
        const int b = __builtin_ctzll(v);
        t2 ^= col[MAXBIT - 1 - b];
        v &= v - 1;
      }
      state[(size_t)d * MAXBIT + j] = t2;
    }
  }
  return PCABO_OK;
}

// n points of a FRESH scrambled Sobol engine (state after pcabo_sobol_scramble, shift = the engine's shift vector), as
// torch.quasirandom.SobolEngine.draw(n, dtype=float64) returns them for num_generated = 0 (first point = float32(shift) / 2^30, then
// Gray-code steps: the state column of the lowest zero bit of the running index is XORed in), mapped into a box as botorch's
// draw_sobol_samples does: out[i][j] = lo[j] + rng[j] * u[i][j] (multiply, then add: two roundings, as torch's two kernels).
// lo = rng = NULL: u itself.
int pcabo_sobol_draw(const int64_t* state, const int64_t* shift, int k, int n, const double* lo, const double* rng, double* out) {
  if (!state || !shift || !out || k < 1 || n < 1 || (lo == nullptr) != (rng == nullptr)) return PCABO_ERR_ARG;
  const int MAXBIT = 30;
  const double recip = 9.31322574615478515625e-10;      // 2^-30
  std::vector<int64_t> q(shift, shift + k);
  for (int i = 0; i < n; ++i) {
    if (i > 0) {
      unsigned v = (unsigned)(i - 1);
      int l = 0;
      while (v & 1u) { v >>= 1; ++l; }
      if (l >= MAXBIT) return PCABO_ERR_ARG;
      for (int j = 0; j < k; ++j) q[j] ^= state[(size_t)j * MAXBIT + l];
    }
    double* o = out + (size_t)i * k;
    for (int j = 0; j < k; ++j) {
      // (torch keeps the FIRST point as `quasi / 2**30` of an int64 tensor: a float32 tensor - that point has 24 bits)
      const double u = i == 0 ? (double)((float)q[j]) * recip : (double)q[j] * recip;
      if (lo) { const double t = rng[j] * u; o[j] = lo[j] + t; }
      else o[j] = u;
    }
  }
  return PCABO_OK;
}


// pcabo_sobol_draw for the runs of a lock-step batch in one call: run r's engine (states[r], shifts[r], ks[r] columns) draws n
// points into outs[r] (n x ks[r], contiguous), mapped into the box whose corners lie in boxes + r * box_stride as [lo(k), hi(k)]
// (the packing pcabo_batch_acq_bounds writes); rng = hi - lo is formed here, the subtraction the caller's numpy made.  A run with
// states[r] == NULL is skipped.  Same numbers as `rows` calls of pcabo_sobol_draw.
int pcabo_sobol_draw_rows(const int64_t* const* states, const int64_t* const* shifts, const int* ks, int rows, int n,
                          const double* boxes, long long box_stride, double* const* outs) {
  if (!states || !shifts || !ks || !boxes || !outs || rows < 1 || n < 1 || n > (1 << 30)) return PCABO_ERR_ARG;
  for (int r = 0; r < rows; ++r)
    if (states[r] && (ks[r] < 1 || !shifts[r] || !outs[r])) return PCABO_ERR_ARG;
  std::vector<double> rng;
  for (int r = 0; r < rows; ++r) {
    if (!states[r]) continue;
    const int k = ks[r];
    const double* lo = boxes + (size_t)r * box_stride;
    rng.resize(k);
    for (int j = 0; j < k; ++j) rng[j] = lo[k + j] - lo[j];
    pcabo_sobol_draw(states[r], shifts[r], k, n, lo, rng.data(), outs[r]);       // (arguments checked above: cannot fail)
  }
  return PCABO_OK;
}

// ---- torch's CPU generator, restated (the host's pacing thread draws the reference's random numbers without torch calls) ----
// The reference's restart heuristic draws from torch's global CPU generator: the Sobol scramble bits (torch.randint(2, ...)) and
// botorch's initialize_q_batch -> torch.multinomial(weights, n, replacement=False) (behind PCA_BO.py:607-614).  With hundreds of
// runs per host thread those two calls were 40 % of the thread's time.  torch's generator is a 32-bit Mersenne Twister
// (at::mt19937: the published MT19937 with `left` / `next` bookkeeping); `blob` is its state exactly as
// torch.Generator.get_state() exports it (CPUGeneratorImplStateLegacy: uint64 seed, int left, int seeded, uint64 next, uint64
// state[624], ...), read and ADVANCED in place, so set_state(blob) puts torch's own generator where torch's own calls would
// have left it.  pcabo/hostrng.py checks both functions against torch when it is imported and falls back to torch on a mismatch.
namespace {
struct TorchMt {
  uint64_t seed; int32_t left; int32_t seeded; uint64_t next; uint64_t state[624];
};
inline uint32_t mt_twist(uint64_t u, uint64_t v) {
  return (uint32_t)((((uint32_t)u & 0x80000000u) | ((uint32_t)v & 0x7fffffffu)) >> 1) ^ (((uint32_t)v & 1u) ? 0x9908b0dfu : 0u);
}
// (index form, blocks shorter than the recurrence's reach of N - M = 227 words: no iteration of a block reads what the block writes
// except st[i + 1] of its last element, read before it is written - the compiler may vectorise)
__attribute__((optimize("O3"))) inline void mt_next_state(TorchMt* s) {
  constexpr int N = 624, M = 397;
  uint64_t* __restrict__ st = s->state;
  for (int i = 0; i < N - M; ++i) st[i] = (uint32_t)st[i + M] ^ mt_twist(st[i], st[i + 1]);
  for (int i = N - M; i < N - 1; ++i) st[i] = (uint32_t)st[i + M - N] ^ mt_twist(st[i], st[i + 1]);
  st[N - 1] = (uint32_t)st[M - 1] ^ mt_twist(st[N - 1], st[0]);
  s->left = N;
  s->next = 0;
}
inline uint32_t mt_draw(TorchMt* s) {
  if (--s->left == 0) mt_next_state(s);
  uint32_t y = (uint32_t)s->state[s->next++];
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}
// the low bit of the tempered words w[0 .. m)
__attribute__((optimize("O3"))) inline void mt_temper_bits(const uint64_t* w, int64_t m, int64_t* out) {
  for (int64_t i = 0; i < m; ++i) {
    uint32_t y = (uint32_t)w[i];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    out[i] = (int64_t)(y & 1u);
  }
}
// The one rule for a state blob of every entry point that draws from it: a seeded generator whose bookkeeping cannot read past
// state[623] - `left` in [1, 624], and either the next draw refills the state (left == 1) or the left - 1 words still to be
// served from `next` on lie inside it (`next` is bounded by itself first: it is the caller's 64 bits, and a sum can wrap).
inline bool mt_blob_ok(const TorchMt* s) {
  return s->seeded && s->left >= 1 && s->left <= 624 && (s->left == 1 || (s->next <= 624 && s->next + (uint64_t)s->left <= 625));
}
}  // namespace

// torch.randint(2, (count,), generator=g): one 32-bit draw per element, value = draw % 2 (int64 out).
int pcabo_torch_randint2(void* blob, int64_t count, int64_t* out) {
  if (!blob || !out || count < 0) return PCABO_ERR_ARG;
  TorchMt* s = static_cast<TorchMt*>(blob);
  if (!mt_blob_ok(s)) return PCABO_ERR_ARG;
  // whole runs of state words at a time (the tempering of a run is a loop without dependencies: the compiler vectorises it);
  // the bookkeeping is mt_draw's: a fresh state serves N draws, `left` stays N after the first of them
  while (count > 0) {
    int64_t take;
    if (s->left == 1) {
      mt_next_state(s);
      take = count < 624 ? count : 624;
      mt_temper_bits(s->state + s->next, take, out);
      s->next += (uint64_t)take;
      s->left = 624 - (int32_t)(take - 1);
    } else {
      take = count < s->left - 1 ? count : s->left - 1;
      mt_temper_bits(s->state + s->next, take, out);
      s->next += (uint64_t)take;
      s->left -= (int32_t)take;
    }
    out += take;
    count -= take;
  }
  return PCABO_OK;
}

namespace {
// The Exp(1) variates of one multinomial draw over n weights, as torch's exponential_ forms them: two draws per element, in index
// order, before any weight is looked at.
void draw_variates(TorchMt* s, int n, double* q) {
  for (int i = 0; i < n; ++i) {
    const uint64_t hi = mt_draw(s), lo = mt_draw(s);
    const uint64_t r64 = (hi << 32) | lo;
    const double u = (double)(r64 & ((1ull << 53) - 1)) * 1.1102230246251565e-16;      // 2^-53
    q[i] = -std::log1p(-u);
  }
}
// the n_pick largest of w_i / q_i, largest first (torch's topk on the ratios), into best[n_pick] and, if given, out; ratio[n] is scratch
void top_ratios(const double* w, const double* q, int n, int n_pick, double* ratio, int* best, int64_t* out) {
  for (int i = 0; i < n; ++i) ratio[i] = w[i] / q[i];
  int have = 0;                        // (n_pick is 10 of 512: selection by insertion)
  for (int i = 0; i < n; ++i) {
    const double v = ratio[i];
    if (have == n_pick && !(v > ratio[best[have - 1]])) continue;
    int pos = have < n_pick ? have : n_pick - 1;
    while (pos > 0 && v > ratio[best[pos - 1]]) { if (pos < n_pick) best[pos] = best[pos - 1]; --pos; }
    best[pos] = i;
    if (have < n_pick) ++have;
  }
  if (out) for (int j = 0; j < n_pick; ++j) out[j] = best[j];
}
// What of botorch's initialize_q_batch stands behind the scores, given the variates of the row's multinomial draw: z = (v - mean) /
// std (unbiased, Welford), weights exp(eta z) (halved exponents while one overflows), the n_pick largest w_i / q_i, the arg-max
// forced into the last place if it was not drawn.  *flag = 0 picked; 1 nothing is picked here - the std is not positive (equal
// values, or a NaN), or ratios tie where the order matters -: torch's own path decides, out is
// left alone, and a caller that drew the variates ahead puts its generator back.  w[n], ratio[n] and best[n_pick] are scratch.
void pick_from_variates(const double* v, const double* q, int n, int n_pick, double eta, double* w, double* ratio, int* best,
                        int64_t* out, int* flag) {
  double mean = 0.0, m2 = 0.0;
  int arg = 0;
  for (int i = 0; i < n; ++i) {
    const double d = v[i] - mean;
    mean += d / (double)(i + 1);
    m2 += d * (v[i] - mean);
    if (v[i] > v[arg]) arg = i;
  }
  const double sd = std::sqrt(m2 / (double)(n - 1));
  if (!(sd > 0.0)) { *flag = 1; return; }
  double scale = eta;
  for (;;) {
    bool inf = false;
    for (int i = 0; i < n; ++i) { w[i] = std::exp(scale * ((v[i] - mean) / sd)); inf = inf || std::isinf(w[i]); }
    if (!inf) break;
    scale *= 0.5;
  }
  top_ratios(w, q, n, n_pick, ratio, best, nullptr);
  // Equal ratios among the picks, or at their lower edge (weights near the largest double over a small variate give several
  // inf; weights that underflowed give several 0): the order torch's topk leaves them in is its own.  Nothing is picked here.
  for (int j = 0; j + 1 < n_pick; ++j)
    if (ratio[best[j]] == ratio[best[j + 1]]) { *flag = 1; return; }
  int at_edge = 0;
  for (int i = 0; i < n; ++i) at_edge += ratio[i] == ratio[best[n_pick - 1]];
  if (at_edge > 1) { *flag = 1; return; }
  for (int j = 0; j < n_pick; ++j) out[j] = best[j];
  bool has = false;
  for (int j = 0; j < n_pick; ++j) has = has || out[j] == arg;
  if (!has) out[n_pick - 1] = arg;
  *flag = 0;
}
}  // namespace

}  // extern "C"

// The pick with its variates drawn ahead (declared in host_side.h).  What a draw can change of a blob is the twister's part of it
// (TorchMt): that much is kept and put back.
bool torch_blob_ok(const void* blob) { return blob && mt_blob_ok(static_cast<const TorchMt*>(blob)); }
AheadPick::AheadPick(int n_, int n_pick_)
    : n(n_), n_pick(n_pick_), before(sizeof(TorchMt)), q((size_t)n_), w((size_t)n_), ratio((size_t)n_), best((size_t)n_pick_) {}
void AheadPick::draw(void* blob_) {
  blob = blob_;
  memcpy(before.data(), blob, sizeof(TorchMt));
  draw_variates(static_cast<TorchMt*>(blob), n, q.data());
}
void AheadPick::put_back() { if (blob) memcpy(blob, before.data(), sizeof(TorchMt)); }
int AheadPick::pick(const double* vals, double eta, int64_t* out) {
  int flag = 1;
  pick_from_variates(vals, q.data(), n, n_pick, eta, w.data(), ratio.data(), best.data(), out, &flag);
  if (flag == 1) put_back();               // (a row without spread draws nothing: its generator goes back as it was)
  return flag;
}

extern "C" {

// botorch's initialize_q_batch for `rows` runs at once (behind PCA_BO.py:607-614): per row z = (v - mean) / std (unbiased), weights
// exp(eta z) (halved exponents while one overflows), torch.multinomial(weights, n_pick) on the row's generator, the arg-max forced
// into the last place if it was not drawn.  flags[r]: 0 picked; 1 all values equal (std == 0: the caller takes botorch's random
// permutation path on torch's generator - nothing was drawn here); 2 row skipped (blobs[r] == NULL).  The statistics are formed
// in this file's order (Welford), not torch's: the weights can differ from a torch-formed row in the last bit, the picks - an
// ordering of weights over independent exponential variates - do not (tests/test_abi_and_host.py compares 10 000 rows).
namespace {
// rows [r0, r1) of pcabo_boltzmann_pick_rows
void boltzmann_rows(void* const* blobs, const double* vals, int r0, int r1, int n, int n_pick, double eta, int64_t* out, int* flags) {
  AheadPick ahead(n, n_pick);
  for (int r = r0; r < r1; ++r) {
    if (!blobs[r]) { flags[r] = 2; continue; }
    ahead.draw(blobs[r]);
    flags[r] = ahead.pick(vals + (size_t)r * n, eta, out + (size_t)r * n_pick);
  }
}
}  // namespace

int pcabo_boltzmann_pick_rows(void* const* blobs, const double* vals, int rows, int n, int n_pick, double eta, int64_t* out, int* flags) {
  if (!blobs || !vals || !out || !flags || rows < 1 || n < 2 || n_pick < 1 || n_pick > n) return PCABO_ERR_ARG;
  for (int r = 0; r < rows; ++r) {
    const TorchMt* s = static_cast<const TorchMt*>(blobs[r]);
    if (s && !mt_blob_ok(s)) return PCABO_ERR_ARG;
  }
  boltzmann_rows(blobs, vals, 0, rows, n, n_pick, eta, out, flags);
  return PCABO_OK;
}

// Debug export, not part of the ABI in include/pcabo.h (tests/test_propose_pick_cpu.py): one row picked as pcabo_propose_acqf
// picks it (AheadPick) - the variates drawn before the scores are handed over, the pick from them, the generator put back when the
// row has no spread (*flag = 1).  put_back != 0: draw, put back, and draw and pick again - the order of pcabo_propose_acqf when
// its scoring fails and the caller comes again.
int pcabo_debug_boltzmann_two_halves(void* blob, const double* vals, int n, int n_pick, double eta, int put_back, int64_t* out, int* flag) {
  if (!vals || !out || !flag || n < 2 || n_pick < 1 || n_pick > n || !torch_blob_ok(blob)) return PCABO_ERR_ARG;
  AheadPick ahead(n, n_pick);
  ahead.draw(blob);
  if (put_back) {
    ahead.put_back();
    ahead.draw(blob);
  }
  *flag = ahead.pick(vals, eta, out);
  return PCABO_OK;
}

// torch.multinomial(weights[r], n_pick, replacement=False, generator=g_r) for `rows` rows with a generator each (blobs[r]; NULL =
// skip the row): q_i = -log1p(-u_i) with u_i = ((hi << 32 | lo) & (2^53 - 1)) 2^-53 from two draws per element (an Exp(1) variate:
// torch's exponential_), picks = the n_pick largest weights[i] / q_i, largest first (torch's topk).  out[rows][n_pick].
int pcabo_torch_multinomial_rows(void* const* blobs, const double* weights, int rows, int n, int n_pick, int64_t* out) {
  if (!blobs || !weights || !out || rows < 1 || n < 1 || n_pick < 1 || n_pick > n) return PCABO_ERR_ARG;
  std::vector<double> ratio((size_t)n), q((size_t)n);
  std::vector<int> best((size_t)n_pick);
  for (int r = 0; r < rows; ++r) {
    TorchMt* s = static_cast<TorchMt*>(blobs[r]);
    if (!s) continue;
    if (!mt_blob_ok(s)) return PCABO_ERR_ARG;
    draw_variates(s, n, q.data());
    top_ratios(weights + (size_t)r * n, q.data(), n, n_pick, ratio.data(), best.data(), out + (size_t)r * n_pick);
  }
  return PCABO_OK;
}

}  // extern "C"
