// The memory of a context as arithmetic, without HIP: its shape (the capacities derived from max_n, max_d, max_q), the layout of its
// two regions as data (every carved buffer's byte offset and element count), and every SECONDARY use of a carved buffer - a feature
// that lives in space another feature owns - as a named function that says where the use starts and how many elements it needs.
// No other file computes a capacity or an offset into a carved buffer.  Included by pcabo_internal.h (so by every translation unit
// of libpcabo.so) and by host_selftest.cpp, which sweeps the shapes under the sanitizers without a GPU: buffers disjoint and
// aligned, every tenant inside its landlord at its largest legal arguments, simultaneous tenants apart, and the offsets pinned to
// a recorded table (the batched kernels address run b's buffers with ONE stride and the bit-pinned tests rest on the layout).
// DESIGN.md "Memory" has the table of tenants.
#pragma once
#include <stddef.h>

// ---- the sizes the layout is made of (shared with the kernels) ---------------------------------------------------------------
#define PCABO_BS 64          // tile edge of the Gram / Cholesky / root-inverse kernels
#define PCABO_SLAB 16        // rows of R handled by one acquisition work-group
#define PCABO_MAXD 128       // largest ambient / reduced dimension supported
#define PCABO_PSTRIDE (2 + 2 * PCABO_MAXD)   // doubles per (query, slab) partial record of the acquisition kernels: |v|^2, mu_s, two gradient parts
#define PCABO_QA_MAX 416      // query coordinates that travel as kernel arguments (3.25 KB; 10 restarts x 40 dims = 400 fit).  With 448 the
                              // kernarg segment of k_acq_fast was exactly HIP's 4096-byte maximum; 416 leaves 256 bytes of head room
#define PCABO_CNT_DONE 0x3fff // capacity of the per-query ticket array
#define PCABO_QFLAG_WORDS 32  // sequence words of the HostMirror, one per query of the largest batch finished inside a launch
                              // (pcabo_internal.h holds PCABO_INLAUNCH_MAXQ to this number)
#define PCABO_GROUP_CNT_OFFSET 8192      // k_acq_group's tickets live in the upper half of the counter array (other slab count)
#define PCABO_HYP_INV_LS 0
#define PCABO_HYP_NOISE 1
#define PCABO_HYP_MEAN_C 2
#define PCABO_HYP_ARD_FOLD 3              // != 0: k_zstats folds this run's ARD lengthscales (read only where ard_ls is given)
#define PCABO_HYP_WORDS 4
// The device optimiser's results in a run's dVal / hVal: the values of the restarts at the head, then eight doubles per restart
// group (k_lbfgsb_group), group gi's at PCABO_OPT_REC_BASE + PCABO_OPT_REC_STRIDE gi.
#define PCABO_OPT_REC_BASE 64
#define PCABO_OPT_REC_STRIDE 8
static_assert(PCABO_QFLAG_WORDS <= PCABO_OPT_REC_BASE, "the values of a call's restarts end in front of the records");
#define PCABO_XQ_TAIL 8                   // doubles of dXq / hXq behind the query block: no kernel reads them (a run's best_f lives in
                                          // dBestF); pcabo_gp_extend counts them into the room for its rows, nothing else may
// The scratch of pcabo_gp_extend / pcabo_gp_truncate (kernels_ext.hip) at the head of a run's dPartial: ks | v | w (NPcap doubles
// each) | small.  small holds the normalised point, its standardised value, the rung and the info word (the header, written by the
// host before the first launch with info 0; the kernels set 1 + index of the point whose pivot failed) and the believer mean's
// partial sums, one per 256 points.
#define EXT_XN 0
#define EXT_YS PCABO_MAXD
#define EXT_HDR_RUNG (PCABO_MAXD + 1)
#define EXT_HDR_INFO (PCABO_MAXD + 2)
#define EXT_HDR 2                          // doubles of the header: rung, info word (an int in the second double)
#define EXT_INFO_SKIP (-1)                 // info word of a run of a batch that takes no part in the call: every kernel leaves it alone
                                           // (never the 1 + index of a failed point, which is positive)
#define EXT_MU (PCABO_MAXD + 3)
#define EXT_MU_MAX 64                      // partial sums: n <= 16384
#define EXT_SMALL (EXT_MU + EXT_MU_MAX)

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// Small results the host needs after a device phase; lives in pinned host memory.
struct HostMirror {
  int k;                 // reduced dimension chosen by the wPCA
  int chol_info;         // 0 or 1 + index of the failing pivot
  int pad0, pad1;
  double y_mean, y_std;
  double norm_lo[PCABO_MAXD], norm_hi[PCABO_MAXD];
  double acq_lo[PCABO_MAXD], acq_hi[PCABO_MAXD];
  volatile unsigned long long qflag[PCABO_QFLAG_WORDS];   // per query: sequence number written after its results
};

// ---- the shape of a context ------------------------------------------------------------------------------------------------
struct CtxShape { int max_n, max_d, max_q, NPcap, DPcap, KPcap, Scap; };
static inline bool ctx_sizes_ok(int max_n, int max_d, int max_q) {
  return max_n >= 2 && max_d >= 1 && max_d <= PCABO_MAXD && max_q >= 1 && max_q < PCABO_CNT_DONE;
}
static inline CtxShape ctx_shape(int max_n, int max_d, int max_q) {
  const int NPcap = round_up(max_n, PCABO_BS);
  return {max_n, max_d, max_q, NPcap, round_up(max_d, 16), round_up(max_d, 4), NPcap / PCABO_SLAB};
}

// ---- the two layouts ---------------------------------------------------------------------------------------------------------
// All device buffers of a context are carved out of ONE allocation (its "region"), all pinned host buffers out of another.  A
// stand-alone context owns both.  The contexts of a batch live side by side in one device slab and one pinned slab with the SAME
// layout, so that buffer X of run b sits at (X of run 0) + b * region bytes: the batched launches address a run's operands as
// `pointer + blockIdx.z * stride` with a single stride for every buffer.  Every buffer starts on a 256-byte boundary, a region
// is a multiple of 4096 bytes.
struct Buf { size_t off, count, elem; };      // byte offset in the region, elements, bytes per element
enum DevBuf { D_X, D_NOISE, D_F, D_WEIGHTS, D_WC, D_RANKS, D_PCAOUT, D_IN, D_C, D_G0, D_G1, D_LAM, D_Z, D_K, D_SWEEPS, D_INFO, D_Y, D_YS,
              D_YSTATS, D_BOUNDS4, D_ZNMEAN, D_USERNB, D_ZNT, D_AT, D_NRM, D_GRAM, D_L, D_R, D_TMP, D_ALPHA, D_DIAG, D_XQ, D_PARTIAL,
              D_VAL, D_GRAD, D_ZQ, D_XOUT, D_BESTF, D_KS, D_COUNTERS, D_MLL, D_ARDLS, D_HYP, D_COUNT };
enum HostBuf { H_MIRROR, H_XQ, H_VAL, H_GRAD, H_SMALL, H_IN, H_BESTF, H_MLL, H_ARDLS, H_HYP, H_COUNT };
struct CtxLayout {
  CtxShape s;
  Buf dev[D_COUNT], host[H_COUNT];
  size_t dev_bytes, host_bytes;               // the regions
};
static inline CtxLayout ctx_layout(const CtxShape& s) {
  CtxLayout L;
  L.s = s;
  const size_t N = s.NPcap, D = s.DPcap, KP = s.KPcap, n = s.max_n, d = s.max_d, Q = s.max_q, nb = N / PCABO_BS, dbl = sizeof(double);
  const size_t mll_shared = nb * (nb + 1), mll_ard = nb * (nb + 1) / 2 * (1 + KP) + KP;     // tile partials of the two forms of the fit
  const struct { int id; size_t elem, count; } dev[D_COUNT] = {
    {D_X, dbl, n * d},           {D_NOISE, dbl, n * d},       {D_F, dbl, n},               {D_WEIGHTS, dbl, n},
    {D_WC, dbl, (n + 4) * D},    {D_RANKS, sizeof(long long), n},
    {D_PCAOUT, dbl, 3 * d + d * d},                           // [data_mean | pca_mean | evr | comps]: pca_parts
    {D_IN, dbl, n * (2 * d + 2)},                             // X, noise, ranks (or f) and y packed: in_pack
    {D_C, dbl, D * D},           {D_G0, dbl, d * d},          {D_G1, dbl, d * d},          {D_LAM, dbl, d},
    {D_Z, dbl, n * d},           {D_K, sizeof(int), 1},       {D_SWEEPS, sizeof(int), 1},  {D_INFO, sizeof(int), 1},
    {D_Y, dbl, n},               {D_YS, dbl, N},              {D_YSTATS, dbl, 2},          {D_BOUNDS4, dbl, 4 * PCABO_MAXD},
    {D_ZNMEAN, dbl, PCABO_MAXD}, {D_USERNB, dbl, 2 * PCABO_MAXD},
    {D_ZNT, dbl, KP * N},        {D_AT, dbl, KP * N},         {D_NRM, dbl, N},
    {D_GRAM, dbl, N * N},        {D_L, dbl, N * N},           {D_R, dbl, N * N},
    {D_TMP, dbl, N},             {D_ALPHA, dbl, N},
    {D_DIAG, dbl, (size_t)2 * PCABO_BS * PCABO_BS},           // two hand-over tiles (k_chol_step)
    {D_XQ, dbl, Q * d + PCABO_XQ_TAIL},
    {D_PARTIAL, dbl, Q * (size_t)s.Scap * PCABO_PSTRIDE},
    {D_VAL, dbl, Q},             {D_GRAD, dbl, Q * d},        {D_ZQ, dbl, d},              {D_XOUT, dbl, d},
    {D_BESTF, dbl, 2},
    {D_KS, dbl, Q * N},                                       // kernel vectors of a large value-only batch (GEMM scoring)
    {D_COUNTERS, sizeof(unsigned int), PCABO_CNT_DONE + 1},
    {D_MLL, dbl, (mll_shared > mll_ard ? mll_shared : mll_ard) + 8},
    {D_ARDLS, dbl, PCABO_MAXD},  {D_HYP, dbl, PCABO_HYP_WORDS},
  };
  const struct { int id; size_t elem, count; } host[H_COUNT] = {
    {H_MIRROR, sizeof(HostMirror), 1},
    // (hXq: at least one QueryArgs block - small batches are handed to the kernel by value from here)
    {H_XQ, dbl, (Q * d > PCABO_QA_MAX ? Q * d : (size_t)PCABO_QA_MAX) + PCABO_XQ_TAIL},
    {H_VAL, dbl, Q},             {H_GRAD, dbl, Q * d},
    {H_SMALL, dbl, d * d + 8 * d + 64},                       // three tenants: small_wpca, small_imap_x, small_norm_bounds
    {H_IN, dbl, n * (2 * d + 2)},
    {H_BESTF, dbl, 2},           {H_MLL, dbl, 8 + KP},        {H_ARDLS, dbl, PCABO_MAXD},  {H_HYP, dbl, PCABO_HYP_WORDS},
  };
  size_t off = 0;
  for (int i = 0; i < D_COUNT; ++i) {         // (the table is in carving order: entry i is buffer i)
    off = (off + 255) & ~(size_t)255;
    L.dev[dev[i].id] = {off, dev[i].count, dev[i].elem};
    off += dev[i].count * dev[i].elem;
  }
  L.dev_bytes = (off + 4095) & ~(size_t)4095;
  off = 0;
  for (int i = 0; i < H_COUNT; ++i) {
    off = (off + 255) & ~(size_t)255;
    L.host[host[i].id] = {off, host[i].count, host[i].elem};
    off += host[i].count * host[i].elem;
  }
  L.host_bytes = (off + 4095) & ~(size_t)4095;
  return L;
}
template <typename T> static inline T* buf_at(char* region, const Buf& b) { return reinterpret_cast<T*>(region + b.off); }

// ---- uses -------------------------------------------------------------------------------------------------------------------
// A use of a buffer: elements [start, start + count) of it.  fits: inside the landlord (a buffer, or a use of one).
struct Use { size_t start, count; };
static inline Use whole(const Buf& b) { return {0, b.count}; }
static inline bool fits(Use u, Use in) { return u.start >= in.start && u.start + u.count <= in.start + in.count; }
static inline bool fits(Use u, const Buf& b) { return fits(u, whole(b)); }
static inline bool apart(Use a, Use b) { return a.start + a.count <= b.start || b.start + b.count <= a.start; }

// dPcaOut, and its copy at the head of hSmall: four parts behind each other
struct PcaParts { size_t data_mean, pca_mean, evr, comps; };
static inline PcaParts pca_parts(const CtxShape& s) { const size_t d = s.max_d; return {0, d, 2 * d, 3 * d}; }
static inline size_t pca_copy_count(const CtxShape& s, int rcount, int d) { return pca_parts(s).comps + (size_t)rcount * d; }   // rcount components of d
// hSmall: the wPCA results, the inverse map's x (a context and the runs of a batch alike), a batch's Normalize bounds on their way
static inline Use small_wpca(const CtxShape& s) { const size_t d = s.max_d; return {0, 3 * d + d * d}; }
static inline Use small_imap_x(const CtxShape& s) { const Use w = small_wpca(s); return {w.start + w.count, (size_t)s.max_d}; }
static inline Use small_norm_bounds(const CtxShape& s) { const Use x = small_imap_x(s); return {x.start + x.count, 2 * (size_t)s.max_d}; }

// dIn / hIn: [X (n x cols) | noise (n x cols) | ranks or f (n) | y (n)], the absent parts left out
struct InPack { size_t noise, ranks, y, total; };
static inline InPack in_pack(int n, int cols, bool noise, bool ranks, bool y) {
  const size_t nc = (size_t)n * cols, r = noise ? 2 * nc : nc, yo = ranks ? r + n : r;
  return {nc, r, yo, y ? yo + n : yo};
}

// dXq / hXq: the query block (max_q points of max_d coordinates) and the tail behind it
static inline Use xq_queries(const CtxShape& s) { return {0, (size_t)s.max_q * s.max_d}; }
// pcabo_gp_extend stages rows of k coordinates and, behind rows_cap of them, their values: as many as fit block and tail
static inline int ext_rows_cap(const CtxShape& s, int k) { return (int)((xq_queries(s).count + PCABO_XQ_TAIL) / ((size_t)k + 1)); }
static inline Use xq_ext_rows(const CtxShape& s, int k) { return {0, (size_t)ext_rows_cap(s, k) * k}; }
static inline Use xq_ext_vals(const CtxShape& s, int k) { return {xq_ext_rows(s, k).count, (size_t)ext_rows_cap(s, k)}; }

// dPartial: the acquisition's slab records are its owner (max_q queries x Scap slabs); the others use what every evaluation writes
// before it reads.  pcabo_gp_extend's scratch, the 4 n leave-one-out results, and the posterior: q (NP / 64) records of the GEMM
// route, then mean | variance | unfloored variance behind them
static inline Use partial_ext_scratch(const CtxShape& s) { return {0, 3 * (size_t)s.NPcap + EXT_SMALL}; }
struct ExtScratch {
  double *ks, *v, *w, *small;
  ExtScratch(double* partial, const CtxShape& s) : ks(partial), v(partial + s.NPcap), w(partial + 2 * (size_t)s.NPcap), small(partial + 3 * (size_t)s.NPcap) {}
};
static inline Use partial_loo(int n) { return {0, 4 * (size_t)n}; }
static inline size_t partial_loo_part(int n, int v) { return (size_t)v * n; }      // v = 0 .. 3: mean | var | z | lpd
static inline Use partial_post_records(int q, int NP) { return {0, (size_t)q * (NP / 64) * PCABO_PSTRIDE}; }
static inline Use partial_post_result(int q, int NP) { return {partial_post_records(q, NP).count, 3 * (size_t)q}; }

// dCounters: the per-query tickets of a launch of q queries, and k_acq_group's (apart while q <= PCABO_GROUP_CNT_OFFSET)
static inline Use counters_queries(int q) { return {0, (size_t)q}; }
static inline Use counters_group() { return {PCABO_GROUP_CNT_OFFSET, PCABO_QFLAG_WORDS}; }

// dGram: K on demand (pcabo_get_gram) is its owner; the device optimiser keeps the transposed root inverse there (NP rows of ld)
static inline Use gram_rt(int NP, int ld) { return {0, (size_t)NP * ld}; }

// dMll: 1 + M partial sums per lower 64 x 64 tile of K^-1 at padded size NP, then the 5 + M results (k_mll_finish; the shared
// lengthscale: M = 1, ARD: M = KP; a batch: one place for all runs, behind the widest run's partials).  hMll: the results
static inline Use mll_partials(int NP, int M) { const size_t nb = NP / PCABO_BS; return {0, (1 + (size_t)M) * (nb * (nb + 1) / 2)}; }
static inline Use mll_result(int NP, int M) { return {mll_partials(NP, M).count, 5 + (size_t)M}; }
static inline Use hmll_result(int M) { return {0, 5 + (size_t)M}; }

// The device optimiser (k_lbfgsb_group) in a run's buffers.  dXq / hXq: [num_restarts x kmax starts | lower | upper] inside the
// query block; dGrad / hGrad: the candidates (mode 0: the gradients); dVal / hVal: the values, then the records of the groups
static inline int opt_groups(int num_restarts, int batch_limit) { return (num_restarts + batch_limit - 1) / batch_limit; }
static inline Use xq_opt_points(int num_restarts, int kmax) { return {0, (size_t)(num_restarts + 2) * kmax}; }
static inline Use grad_opt_cands(int num_restarts, int kmax) { return {0, (size_t)num_restarts * kmax}; }
static inline Use val_opt_values(int num_restarts) { return {0, (size_t)num_restarts}; }
static inline Use val_opt_records(int ngroups) { return {PCABO_OPT_REC_BASE, (size_t)PCABO_OPT_REC_STRIDE * ngroups}; }
static inline size_t val_opt_record(int gi) { return PCABO_OPT_REC_BASE + (size_t)PCABO_OPT_REC_STRIDE * gi; }      // group gi's eight doubles
// Has a run room for a call of the device optimiser (mode 0 keeps no records: ngroups = 0)?
static inline bool opt_fits(const CtxLayout& L, int num_restarts, int ngroups, int kmax) {
  return fits(val_opt_records(ngroups), L.dev[D_VAL]) && fits(xq_opt_points(num_restarts, kmax), xq_queries(L.s));
}
