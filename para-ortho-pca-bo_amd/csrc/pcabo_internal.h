// Internal declarations shared by the HIP translation units of libpcabo.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "ctx_layout.h"      // the sizes, HostMirror, round_up and where everything lies in a context's memory (no HIP in there)

#define PCABO_TLD 66         // LDS leading dimension (doubles) of a 64x64 tile: conflict-free ds_read_b64
#define PCABO_INLAUNCH_MAXQ 32 // largest batch finished inside the launch (results + flags straight to the host)
static_assert(PCABO_INLAUNCH_MAXQ == PCABO_QFLAG_WORDS, "one sequence word of the host mirror per query finished inside a launch");

typedef double double4_t __attribute__((ext_vector_type(4)));
struct QueryArgs { double x[PCABO_QA_MAX]; };
// Mailbox of the resident ("server") acquisition kernel: (value, tag) pairs of 16 bytes.  A pair is written value
// first, tag second (one 16-byte store on the device) and read as one 16-byte snapshot, so a matching tag implies the
// value.  Pair 0 is the header (value = number of queries of the round, 0 = leave), pairs 1.. the query coordinates.
struct alignas(16) MailPair { double v; unsigned long long tag; };
// Pairs WRITTEN BY THE HOST carry tag = sequence number XOR mail_mix(bits of the value): a reader that sees a pair torn
// between two rounds (new tag, old value - possible in principle when a write-combining buffer of the host is flushed in
// pieces) computes a different sequence number and simply polls again.
static inline __host__ __device__ unsigned long long mail_mix(unsigned long long vbits) {
  const unsigned int lo = (unsigned int)vbits, hi = (unsigned int)(vbits >> 32);
  return (unsigned long long)((lo ^ hi ^ (hi >> 11)) & 0xFFFFFFu);
}
#define PCABO_MAIL_PAIRS (1 + PCABO_QA_MAX + PCABO_INLAUNCH_MAXQ + 1)   // [0] unused, coordinates, one control pair per query, probe
#define PCABO_SERVER_TIMEOUT_TICKS 200000000ull // 2 s of wall_clock64 (100 MHz): every wait in the kernel is bounded

#ifdef __HIPCC__
// fp64 reciprocal / reciprocal square root from the hardware estimate (v_rcp_f64 / v_rsq_f64) plus two
// Newton steps: <= 2 ulp, ~6 instructions instead of the ~25-40 of an IEEE divide / sqrt sequence.  Used where
// a sequential dependency chain makes instruction count the bottleneck (panel factorisation, Jacobi rotations).
__device__ inline double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}
__device__ inline double fast_rsq(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * fma(-0.5 * x * y, y, 1.5);
  y = y * fma(-0.5 * x * y, y, 1.5);
  return y;
}
#endif

// Model / problem constants handed to the acquisition kernels by value.
struct AcqParams {
  double best_f;        // already rounded like torch.as_tensor(float) does; PCABO_ACQ_UCB: the slot carries kappa = sqrt(beta)
  double y_mean, y_std; // filled on device from the standardisation kernel (host copy unused)
  double inv_ls;        // 1 / lengthscale
  int maximize;
  int acq;              // PCABO_ACQ_*
  int kernel;           // PCABO_KERNEL_*
  int want_grad;
};

// The conditioned model as the acquisition launchers read it: the sizes and the device operands of a context, or of run 0 of a
// batch with the batch's n / NP and the largest k of its runs (gp_model in pcabo_api.hip builds both).
struct GpModel { int n, k, NP, ld; const double *ZnT, *R, *alpha, *bounds4, *ystats; };

// Batched acquisition launches (all zero / null for a single context).  Runs are addressed as in zrun(); per run the
// reduced dimension and best_f come from device memory (they differ between the runs of a batch).
struct AcqBatch {
  size_t zs = 0, hzs = 0;          // strides of the device region / the pinned host region
  const int* k_dev = nullptr;      // run 0's dK      (null: the k argument)
  const double* bestf = nullptr;   // run 0's dBestF  (null: prm.best_f)
  int table = 0;                   // 1: blockIdx.y indexes the active-query table that travels in the QueryArgs slot
                                   //    (32-bit entries: run << 16 | query of that run); 0: run = blockIdx.z
  int xq_host = 0;                 // 1: Xq is a pinned HOST pointer (stride hzs), read by the kernel over PCIe
  const double* hyp = nullptr;     // run 0's hyperparameter block (PCABO_HYP_*) after a lock-step fit (null: prm.inv_ls)
};

// ---- launchers (defined in kernels_*.hip); all asynchronous on `s` -------------------
#if defined(__HIPCC__)
// 16-byte loads / stores that go to the fabric (system scope: no L1/L2 copy is trusted or left behind)
typedef unsigned int pcabo_u4 __attribute__((ext_vector_type(4)));
__device__ inline pcabo_u4 ld_pair_sys(const void* p) {
  pcabo_u4 r;
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
  return r;
}
__device__ inline void st_pair_sys(void* p, pcabo_u4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
}
// up to 8 pair loads in flight, one wait (cnt <= 8; unused slots repeat slot 0)
__device__ inline void ld_pairs_sys8(const void* const* p, pcabo_u4* o) {
  asm volatile(
      "global_load_dwordx4 %0, %8, off sc0 sc1\n\tglobal_load_dwordx4 %1, %9, off sc0 sc1\n\t"
      "global_load_dwordx4 %2, %10, off sc0 sc1\n\tglobal_load_dwordx4 %3, %11, off sc0 sc1\n\t"
      "global_load_dwordx4 %4, %12, off sc0 sc1\n\tglobal_load_dwordx4 %5, %13, off sc0 sc1\n\t"
      "global_load_dwordx4 %6, %14, off sc0 sc1\n\tglobal_load_dwordx4 %7, %15, off sc0 sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
      : "memory");
}
__device__ inline pcabo_u4 make_pair(double v, unsigned long long tag) {
  pcabo_u4 r;
  r.x = (unsigned int)__double2loint(v); r.y = (unsigned int)__double2hiint(v);
  r.z = (unsigned int)(tag & 0xffffffffull); r.w = (unsigned int)(tag >> 32);
  return r;
}
__device__ inline unsigned long long pair_tag(pcabo_u4 v) { return ((unsigned long long)v.w << 32) | v.z; }
__device__ inline double pair_value(pcabo_u4 v) { return __hiloint2double((int)v.y, (int)v.x); }
// sequence number of a host-written pair (see mail_mix)
__device__ inline unsigned long long mail_seq(pcabo_u4 v) {
  return pair_tag(v) ^ mail_mix(((unsigned long long)v.y << 32) | v.x);
}

// Batched launches (pcabo_batch_*): blockIdx.z = run.  The contexts of a batch share one layout, so run b's copy of any
// device buffer sits b * zs bytes behind run 0's (b * hzs for the pinned host mirror).  zs = 0 / gridDim.z = 1 otherwise.
// (plain pointer arithmetic on the kernel argument, no detour through an integer: the compiler then still knows the
// result points to GLOBAL memory and emits global_load/global_store; through uintptr_t it falls back to flat_* accesses,
// which also count on the LDS counter - every LDS wait then waits for the global loads in flight as well)
template <typename T>
__device__ inline T* zrun(T* p, size_t stride, unsigned run) {
  typedef typename std::remove_const<T>::type U;
  return p ? reinterpret_cast<T*>(reinterpret_cast<char*>(const_cast<U*>(p)) + (size_t)run * stride) : p;   // (NULL stays NULL)
}
#define ZRUN(p) p = zrun(p, zs, blockIdx.z)

// XCD-aware placement of a batched launch (grid (gx, gy, B), B runs of gx * gy tiles each).  Work-groups are dealt round-robin
// over the 8 XCDs in dispatch order (x fastest), so the tiles of ONE run land on eight different L2s and every XCD fetches
// the operand tiles those work-groups share (the block row L[J][.] of a look-back, the diagonal block of a panel, the L
// tiles a column chunk of the root inverse walks) for itself.  The linear work-group id is read as (run, tile) such that all
// tiles of a run have the same id % 8: one XCD, one L2 copy of the shared operands.  Placement only - every (run, tile)
// pair is still visited exactly once, whatever the hardware does with the ids; runs beyond the last multiple of 8 (and
// single contexts) keep the identity mapping.
struct XcdTile { unsigned run, x, y; };
#if defined(__HIPCC__)
__device__ inline XcdTile xcd_tile() {
  const unsigned gx = gridDim.x, gy = gridDim.y, T = gx * gy;
  const unsigned lin = (blockIdx.z * gy + blockIdx.y) * gx + blockIdx.x, full = (gridDim.z & ~7u) * T;
  XcdTile t;
  if (lin < full) {
    const unsigned slot = lin >> 3, tile = slot % T;
    t.run = (slot / T) * 8u + (lin & 7u); t.x = tile % gx; t.y = tile / gx;
  } else { t.run = blockIdx.z; t.x = blockIdx.x; t.y = blockIdx.y; }
  return t;
}
#endif
#define ZRUNX(p) p = zrun(p, zs, xt_.run)

// Wave-wide sum without LDS traffic.  `__shfl_xor` compiles to ds_bpermute_b32 (two per double, each followed by an
// lgkmcnt wait: ~100 cycles of dependent latency per step); in a kernel whose whole budget is ~15 us the reductions
// were the largest single item.  DPP steps stay inside the VALU: quad_perm x2, row_half_mirror, row_mirror leave the
// row sum in all 16 lanes; row_bcast15 / row_bcast31 carry it across the four rows into lane 63.
template <int CTRL, int ROW_MASK>
__device__ inline double dpp_get(double v) {
  int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
// The same move for a permutation INSIDE a row with every row and bank enabled (quad_perm, row_half_mirror, row_mirror, row_ror):
// each lane has a valid source, so no lane keeps `old`.  bound_ctrl says so to the compiler, which then drops the two
// `v_mov_b32 v, 0` (and often an s_nop) that every dpp_get costs for filling `old`.
template <int CTRL>
__device__ inline double dpp_row(double v) {
  int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ inline double row_sum16(double v) {        // every lane: sum over its row of 16 lanes
  v += dpp_get<0xB1, 0xf>(v);      // quad_perm [1,0,3,2]
  v += dpp_get<0x4E, 0xf>(v);      // quad_perm [2,3,0,1]
  v += dpp_get<0x141, 0xf>(v);     // row_half_mirror
  v += dpp_get<0x140, 0xf>(v);     // row_mirror
  return v;
}
__device__ inline double wave_sum(double v) {         // uniform result: sum over all 64 lanes
  v = row_sum16(v);
  v += dpp_get<0x142, 0xa>(v);     // row_bcast15 -> rows 1, 3
  v += dpp_get<0x143, 0xc>(v);     // row_bcast31 -> rows 2, 3
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63),
                          __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// The LDS-staged 64 x 64 fp64 tile product of a work-group of 256 (k_score_gemm, k_post_cov, k_post_sample): `steps` steps of
// depth 64, the operand tiles of a step through s_a / s_b (64 x PCABO_TLD doubles each), the next step's tiles travelling in
// registers while the MFMAs of the current one run.  elem(step, r, c, a, b) names element (r, c) of the step's two tiles: the
// caller's addressing, bounds guards and masks live there.  Wave w's acc[t] accumulates, steps and kk ascending,
//   KMAJOR = false  sum_j s_a[16 w + i][j] s_b[16 t + i'][j]     (tiles [row][depth])
//   KMAJOR = true   sum_j s_a[j][16 w + i] s_b[j][16 t + i']     (tiles [depth][row])
// as acc[t][r] = result[16 w + (l >> 4) + 4 r][16 t + (l & 15)].  One MFMA order per accumulator for every caller: that order is
// what gives |v|^2 the same bits in the scoring and in the posterior.  s_a / s_b may be reused after a barrier.
template <bool KMAJOR, typename Elem>
__device__ __forceinline__ void tile_product_f64(double* s_a, double* s_b, int steps, Elem elem, double4_t (&acc)[4]) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  double pa[16], pb[16];
  auto fetch = [&](int J) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int idx = tid + 256 * u;
      elem(J, idx >> 6, idx & 63, pa[u], pb[u]);
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int idx = tid + 256 * u, r = idx >> 6, c = idx & 63;
      s_a[r * PCABO_TLD + c] = pa[u];
      s_b[r * PCABO_TLD + c] = pb[u];
    }
  };
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
  fetch(0);
  for (int J = 0; J < steps; ++J) {
    __syncthreads();                          // the previous step's MFMAs have read the LDS tiles
    put();
    if (J + 1 < steps) fetch(J + 1);
    __syncthreads();
    for (int kk = 0; kk < 64; kk += 4) {
      const double a = KMAJOR ? s_a[(kk + (l >> 4)) * PCABO_TLD + 16 * w + (l & 15)]
                              : s_a[(16 * w + (l & 15)) * PCABO_TLD + kk + (l >> 4)];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double b = KMAJOR ? s_b[(kk + (l >> 4)) * PCABO_TLD + 16 * t + (l & 15)]
                                : s_b[(16 * t + (l & 15)) * PCABO_TLD + kk + (l >> 4)];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
      }
    }
  }
}

// ---- N sums at once, bit for bit those of N wave_sum calls ----------------------------------------------------------
// wave_sum adds the lanes as a balanced binary tree in lane order: level t adds the sums of lane blocks that differ in
// lane bit t (f64 addition is commutative, so which of the two lanes holds which operand does not change a bit).  The
// multi-value form builds the same tree for every value but transposes the work, like a reduce-scatter: at level t the
// live values of a lane are taken in pairs; lanes with bit t clear keep the first of a pair, lanes with bit t set the
// second, and each lane adds its partner's (lane ^ 2^t) partial of the value it keeps.  The number of live values halves
// per level (an odd one out is added symmetrically), so N values cost ~7 N wave instructions instead of ~20 N, and the
// N sums end up in N different lanes (wave_multi_owner), ready for one store instruction.
template <int T>
__device__ inline double lane_xor(double v) {           // v of lane l ^ 2^T, T < 4 (DPP, inside a row of 16)
  if (T == 0) return dpp_get<0xB1, 0xf>(v);             // quad_perm [1,0,3,2]
  if (T == 1) return dpp_get<0x4E, 0xf>(v);             // quad_perm [2,3,0,1]
  if (T == 2) return dpp_get<0x141, 0xf>(dpp_get<0x1B, 0xf>(v));   // quad_perm [3,2,1,0], then row_half_mirror: l ^ 4
  return dpp_get<0x128, 0xf>(v);                        // row_ror 8: l ^ 8
}
// v_permlane16_swap (T = 4) / v_permlane32_swap (T = 5): the lanes with bit T set of a trade places with the lanes with
// bit T clear of b, so a + b afterwards is a's level-T sum where bit T is clear and b's where it is set.  No select.
template <int T>
__device__ inline double swap_add(double a, double b) {
  unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
  unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
  if (T == 4) {
    const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    alo = lo[0]; blo = lo[1]; ahi = hi[0]; bhi = hi[1];
  } else {
    const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    alo = lo[0]; blo = lo[1]; ahi = hi[0]; bhi = hi[1];
  }
  return __hiloint2double((int)ahi, (int)alo) + __hiloint2double((int)bhi, (int)blo);
}
template <int T>
__device__ inline double pair_level(double a, double b, int lane) {   // bit T clear: a's level-T sum; set: b's
  if (T >= 4) return swap_add<T>(a, b);
  const bool hi = (lane >> T) & 1;
  return (hi ? b : a) + lane_xor<T>(hi ? a : b);
}
template <int T>
__device__ inline double single_level(double v) {       // every lane: its level-T sum of v
  if (T >= 4) return swap_add<T>(v, v);
  return v + lane_xor<T>(v);
}
__host__ __device__ constexpr int wave_multi_live(int n, int t) { return (n + (1 << t) - 1) >> t; }   // values before level t: ceil(n / 2^t)
template <int T, int N>
__device__ inline void wave_multi_level(double* v, int lane) {
  constexpr int M = wave_multi_live(N, T);
#pragma unroll
  for (int i = 0; i < M / 2; ++i) v[i] = pair_level<T>(v[2 * i], v[2 * i + 1], lane);
  if (M & 1) v[M / 2] = single_level<T>(v[M - 1]);
}
// v[0 .. N) per lane -> v[0] = the wave sum of value wave_multi_index<N>(lane) (N <= 64; v[1 ..] are left undefined)
template <int N>
__device__ inline void wave_sum_multi(double* v, int lane) {
  static_assert(N >= 1 && N <= 64, "one value per lane at the end");
  wave_multi_level<0, N>(v, lane); wave_multi_level<1, N>(v, lane); wave_multi_level<2, N>(v, lane);
  wave_multi_level<3, N>(v, lane); wave_multi_level<4, N>(v, lane); wave_multi_level<5, N>(v, lane);
}
// which value's sum this lane holds after wave_sum_multi<N> ...
template <int N>
__device__ inline int wave_multi_index(int lane) {
  int slot = 0;
#pragma unroll
  for (int t = 5; t >= 0; --t) {
    const int m = wave_multi_live(N, t);
    slot = slot < m / 2 ? 2 * slot + ((lane >> t) & 1) : m - 1;
  }
  return slot;
}
// ... and whether it is the one lane that publishes it (values added symmetrically at some level sit in several lanes)
template <int N>
__device__ inline int wave_multi_owner(int lane) {
  int slot = 0;
  bool first = true;
#pragma unroll
  for (int t = 5; t >= 0; --t) {
    const int m = wave_multi_live(N, t);
    if (slot < m / 2) slot = 2 * slot + ((lane >> t) & 1);
    else { slot = m - 1; first = first && !((lane >> t) & 1); }
  }
  return first ? slot : -1;
}
// the lane that owns value i, for a uniform copy through readlane (use it in a constant expression)
__host__ __device__ constexpr int wave_multi_lane(int n, int i, int t = 0) {
  return t == 6 ? 0
       : (i < wave_multi_live(n, t) / 2 * 2 ? ((i & 1) << t) + wave_multi_lane(n, i / 2, t + 1)
                                            : wave_multi_lane(n, wave_multi_live(n, t) / 2, t + 1));
}
__device__ inline double read_lane(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}
#endif

void launch_rank(hipStream_t s, const double* f, int n, int maximize, long long* ranks);
// B > 1: batched launch over the B contexts of a batch (blockIdx.z = run, buffer strides zs / hzs bytes, see zrun)
// hyp: run 0's hyperparameter block, set once the runs of a batch carry their own fitted model (pcabo_batch_gp_fit): k_zstats,
// k_znorm and k_gram then read the mean constant, 1 / lengthscale and the noise of THEIR run from it instead of the scalar
// argument.  The host writes the very doubles the single-context path passes by value (1.0 / softplus(rho) is formed there).
// (the words of a block: PCABO_HYP_* in ctx_layout.h)
struct ZB { int B = 1; size_t zs = 0, hzs = 0; const double* hyp = nullptr; };
void launch_wpca_prep(hipStream_t s, const double* X, const long long* ranks, const double* noise, int n, int d,
                      int DP, double* weights, double* data_mean, double* pca_mean, double* Wc, ZB zb = ZB());
void launch_cov(hipStream_t s, const double* Wc, int n, int DP, double* C, ZB zb = ZB());
// eigen-decomposition + selection (components sorted by variance, evr, k, sign rule) in one launch
void launch_jacobi(hipStream_t s, const double* C, int d, int DP, const double* V0, double* G, double* lam, int* sweeps,
                   int n, double var_threshold, int n_components, double* comps, double* evr, int* k_dev, HostMirror* hm,
                   ZB zb = ZB());
void launch_project(hipStream_t s, const double* X, const double* data_mean, const double* pca_mean,
                    const double* comps, const int* k_dev, int n, int d, double* Z, ZB zb = ZB());
void launch_zstats(hipStream_t s, const double* Z, const double* y, int n, int k, const double* user_norm_bounds,
                   double* bounds4 /*norm_lo,norm_hi,acq_lo,acq_hi each MAXD*/, double* zn_mean, double* ystats,
                   double* ys, HostMirror* hm, const int* k_dev = nullptr, ZB zb = ZB(),
                   double mean_c = 0.0,    // mean_c: constant mean of a fitted GP (y_s and the statistics carry m + s c)
                   const double* ard_ls = nullptr);   // ARD fit: k lengthscales on the device, folded into the Normalize ranges
                                                      // (norm_hi = norm_lo + (norm_hi - norm_lo) l_c; null: nothing changes).
                                                      // Batched: run b's lie zb.zs bytes further per run and are folded only
                                                      // where word PCABO_HYP_ARD_FOLD of its zb.hyp block is non-zero
void launch_znorm(hipStream_t s, const double* Z, int n, int k, int NP, int KP, int ld, const double* bounds4,
                  const double* zn_mean, double inv_ls, double* ZnT, double* AT, double* nrm,
                  const int* k_dev = nullptr, ZB zb = ZB());   // k_dev != NULL: k (and KP) are read on the device, the arguments ignored
void launch_gram(hipStream_t s, const double* AT, const double* nrm, int n, int NP, int KP, int ld, double noise,
                 int kernel, double* K, const int* k_dev = nullptr, double* K2 = nullptr, int* info_reset = nullptr,
                 ZB zb = ZB());
void launch_add_jitter(hipStream_t s, double* K, int n, int ld, double jitter);
// 0, or -1 when nothing was factored (the device or a kernel attribute could not be set up)
// R_folded != null (one run, chol_step_form(NP, zb) only): the root inverse is computed beside the panels, all but its last row
// block - launch_trinv_drain instead of launch_trinv behind it
int launch_cholesky(hipStream_t s, double* L, int NP, int ld, int* info, double* diag_scratch, ZB zb = ZB(), double* R_folded = nullptr);
bool chol_step_form(int NP, ZB zb);
void launch_trinv_drain(hipStream_t s, const double* L, int NP, int ld, double* R);
void launch_trinv(hipStream_t s, const double* L, int NP, int ld, double* R, ZB zb = ZB());
void launch_chol_panel(hipStream_t s, double* L, int p, int nblocks, int ld, int* info, double* diag_scratch, ZB zb = ZB());
int launch_chol_steps(hipStream_t s, double* L, int NP, int ld, int* info, double* diag_scratch /* two tiles */, ZB zb = ZB(),
                      double* R = nullptr);
void launch_trinv_diag_w(hipStream_t s, const double* L, int nblk, int ld, double* R, ZB zb = ZB());
void launch_alpha(hipStream_t s, const double* R, const double* ys, int n, int NP, int ld, double* tmp, double* alpha,
                  ZB zb = ZB());
// The same two launches for the runs of a batch of which some take no part: gate = run 0's gate word (the others zb.zs bytes apart
// each); a run whose word is not 0 keeps its tmp and alpha bytes, a run whose word is 0 gets launch_alpha's bits.
void launch_alpha_gated(hipStream_t s, const double* R, const double* ys, int n, int NP, int ld, double* tmp, double* alpha, ZB zb,
                        const int* gate);
// marginal-likelihood pieces of a conditioned state (kernels_fit.hip, Matern-5/2): partial = 1 + M doubles per lower 64 x 64 tile,
// out[5 + M] = {sum log L_ii, y_s^T alpha, sum alpha, alpha^T alpha, tr K^-1, then M sums}.  The shared lengthscale: M = 1,
// sum_ij W_ij dK_ij/dlog l.  ard (one lengthscale per input, folded into the Normalize ranges): M = KP, S_c = sum_ij W_ij
// dK_ij/dlog l_c for c < KP.
// zb.B > 1: one launch pair for the B runs of a batch (blockIdx.z = run, k / KP of a run from k_dev, n and NP common)
void launch_mll_grad(hipStream_t s, bool ard, const double* R, const double* AT, const double* nrm, const double* alpha,
                     const double* L, const double* ys, int n, int NP, int KP, int ld, double* partial, double* out,
                     const int* k_dev = nullptr, ZB zb = ZB());
void launch_acq(hipStream_t s, const QueryArgs* qa, const double* Xq, int q, const GpModel& m, AcqParams p, double* partial,
                unsigned int* counters, double* val, double* grad, double* host_val, double* host_grad, HostMirror* hm,
                unsigned long long seq,
                MailPair* dev_mail = nullptr, MailPair* part_pairs = nullptr,
                AcqBatch ab = AcqBatch(), int B = 1, int table_entries = 0);
// throughput variant: one work-group per (restart group of <= 5 queries, 64-row slab); `tab` holds `entries` 32-bit words
// run << 16 | first query << 8 | count (see k_acq_group)
#define PCABO_GROUP_Q 5
bool acq_group_possible(int NP, int k);
int launch_acq_group(hipStream_t st, const QueryArgs* tab, int entries, const double* Xq, const GpModel& m, AcqParams p,
                     double* partial, unsigned int* counters, double* val, double* grad, double* host_val, double* host_grad,
                     HostMirror* hm, unsigned long long seq, AcqBatch ab);   // 0, or -1: nothing launched
// value-only scoring of a large batch as a GEMM (KS, then V = R KS^T on MFMA, then the scalar chain); KS: q x ld scratch
bool score_gemm_possible(int q);
void launch_score(hipStream_t st, const double* Xq, int q, const GpModel& m, AcqParams p, double* KS, double* partial, double* val,
                  AcqBatch ab = AcqBatch(), int B = 1);
// launch_score's first kernel without its mu_s sums (no alpha), and the rest of launch_score behind it: together launch_score's bits
// (launch_score_ks_only reads the model's ZnT and bounds4 only: alpha and R may still be in the making)
void launch_score_ks_only(hipStream_t st, const double* Xq, int q, const GpModel& m, AcqParams p, double* KS);
// launch_score's first kernel alone, for any q >= 1 (launch_posterior starts with it)
void launch_score_ks(hipStream_t st, const double* Xq, int q, const GpModel& m, AcqParams p, double* KS, double* partial,
                     AcqBatch ab = AcqBatch(), int B = 1);
// The scoring's second kernel alone: V = R KS^T on MFMA, its column norms into the partial records; grid (NP / 64, ceil(q / 64), B).
// V (NP x q, runs vzs bytes apart) given: the instantiation that also stores it (launch_posterior with a covariance).
void launch_score_gemm(hipStream_t st, const GpModel& m, int q, const double* KS, double* partial, size_t zs = 0, int B = 1,
                       double* V = nullptr, size_t vzs = 0);
// Posterior mean / variance / covariance at q >= 1 points (kernels_post.hip; KS and partial are the scoring's workspaces):
// post[3 q] = mean | variance (floored) | variance before the floor; V (NP x q) and cov (q x q) both given or both null.
// s2: the likelihood noise (a batch after its fit: read from ab.hyp); vzs: bytes between two runs' V / cov blocks.
void launch_posterior(hipStream_t st, const double* Xq, int q, const GpModel& m, AcqParams p, double s2, int obs_noise,
                      double* KS, double* partial, double* post, double* V, double* cov, AcqBatch ab = AcqBatch(),
                      size_t vzs = 0, int B = 1);
// Joint samples behind launch_posterior's covariance (kernels_post.hip): F (QP x QP, QP = 64 ceil(q / 64)) = cov + jitter s_y^2 I,
// identity on the padding, *info = 0 - ready for launch_cholesky(F, QP, QP, info, ...); then out (S x q) = [mean +] base (S x q) Lc^T
// from the factored F.  zs: the runs' context stride (ystats, mean), vzs: between their cov blocks, szs: between their sample blocks.
void launch_post_chol_prep(hipStream_t st, const double* cov, int q, const double* ystats, double jitter, double* F, int* info,
                           size_t zs = 0, size_t vzs = 0, size_t szs = 0, int B = 1);
void launch_post_sample(hipStream_t st, const double* F, int q, const double* base, int S, const double* mean /* or null */,
                        double* out, size_t zs = 0, size_t szs = 0, int B = 1);
// Leave-one-out predictions of the conditioned GP (kernels_post.hip): out[4 n] = mean | var | z | lpd from R, alpha, the standardised
// targets ys and ystats = (m', s); one launch, grid (ceil(n / 64), 1, B), the runs of a batch zs bytes apart.
void launch_loo(hipStream_t st, const double* R, const double* alpha, const double* ys, const double* ystats, int n, int ld,
                double* out, size_t zs = 0, int B = 1);
// Appending points to a conditioned GP and taking them back (kernels_ext.hip).  The scratch of a run lies at the head of its
// dPartial, which every evaluation writes before it reads (ExtScratch and the EXT_* words of its small block: ctx_layout.h).
// m: the model BEFORE the point (n, NP); X / Y: the staged points and values of the call, row xi / entry yi this one's (Y null:
// believer mode, the value is the model's mean there).  launch_alpha(R, e.ks, n, NP, ld, e.v, e.w) goes between the two.
// GpArrays: the arrays of a run (run 0 of a batch) that an appended point or a take-back writes, and zn_mean, which the append reads.
struct GpArrays { const double* zn_mean; double *L, *R, *ZnT, *AT, *nrm, *ys; };
void launch_ext_ks(hipStream_t st, const double* X, int xi, const double* Y, int yi, const GpModel& m, double inv_ls, int kernel,
                   const ExtScratch& e, AcqBatch ab = AcqBatch(), int B = 1);
void launch_ext_append(hipStream_t st, const GpModel& m, const ExtScratch& e, int idx, int believer, double s2, double inv_ls,
                       const GpArrays& a, AcqBatch ab = AcqBatch(), int B = 1);
// NP: the padded size before the call
void launch_ext_truncate(hipStream_t st, const ExtScratch& e, int n0, int k, int NP, int ld, const GpArrays& a,
                         AcqBatch ab = AcqBatch(), int B = 1);
void launch_score_tail(hipStream_t st, int q, const GpModel& m, AcqParams p, const double* KS, double* partial, double* val);
// resident mode available for this shape? (fast path + every group of the grid co-resident)
bool acq_server_possible(int q, int n, int k, int NP);
int acq_slabs(int NP);
void launch_inverse_map(hipStream_t s, const double* z, const double* comps, const double* data_mean,
                        const double* pca_mean, int k, int d, double* x, const int* k_dev = nullptr, ZB zb = ZB(),
                        double* host_x = nullptr, HostMirror* hm = nullptr, unsigned long long seq = 0);   // host_x / hm: results + flag to pinned host
// Device-resident L-BFGS-B of a batch's restart groups (kernels_lbfgsb.hip): RT = transposed root inverse (zeros above the
// diagonal and beyond n), then one work-group per table entry (run << 16 | first query << 8 | count).  mode 1: optimise from the
// initial conditions in Xq ([num_restarts x k | lower k | upper k] per run), candidates to out_x, values / counters to out_v (the
// eight counters of the group that starts at restart gi batch_limit at out_v + PCABO_OPT_REC_BASE + PCABO_OPT_REC_STRIDE gi);
// mode 0: one value+gradient evaluation at the points in Xq.  Returns 0, or -1 when the launch could not be set up.
void launch_rt_build(hipStream_t s, const double* R, int n, int NP, int ld, double* RT, ZB zb = ZB());
bool lbfgsb_device_possible(int NP, int kmax, int batch_limit);
// (m.k is not read: every run's k comes from k_dev)
int launch_lbfgsb_group(hipStream_t st, const unsigned* table, int entries, int mode, int num_restarts, int maxiter, const GpModel& m,
                        const double* Xq, const double* RT, const double* bestf, const int* k_dev, double inv_ls,
                        int maximize, int acq, int kernel, double* out_x, double* out_v, size_t zs,
                        const double* hyp = nullptr,    // hyp: per-run hyperparameter blocks (stride zs), 1 / lengthscale read from them
                        int batch_limit = PCABO_GROUP_Q);   // mode 1: restarts per group of the call (group gi starts at gi batch_limit)
