// Marginal-likelihood gradient of the exact GP on gfx950 (opt-in hyperparameter fit, DESIGN.md "GP hyperparameter fit").
//
// At a conditioned state (L = chol(K), R = L^-1, alpha = K^-1 y_s, all from kernels_gp.hip) the fit needs, besides the scalar
// pieces of the loss, the two contractions
//   tr K^-1                       and   S = sum_ij W_ij dK_ij/dlog l,   W = alpha alpha^T - K^-1,
// where dK/dlog l = (5/3) r^2 (1 + sqrt5 r) exp(-sqrt5 r) for Matern-5/2 (0 on the diagonal).  K^-1 = R^T R is formed tile by
// tile on f64 MFMA and consumed in the epilogue: it never goes to memory.
//
// Storage as in kernels_gp.hip: R is NP x NP row-major (leading dimension ld), lower triangular, identity on the padding.
#include "pcabo_internal.h"

#define BS PCABO_BS

// Tile t of the lower triangle: t = I (I + 1) / 2 + J, 0 <= J <= I.
struct MllTile { int I, J; };
__device__ __forceinline__ MllTile mll_tile(int t) {
  int I = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  return MllTile{I, t - I * (I + 1) / 2};
}
// acc = this wave's 16 x 64 part of the K^-1 tile (ci: first column of its A rows, cj: of the tile's B columns; rows p0 .. NP - 1 of
// R, a multiple of 64 rows, 16 rows per trip: 20 loads in flight per lane);  dd = the same part of AT^T AT, exactly as k_gram forms it
__device__ __forceinline__ void mll_tile_products(const double* __restrict__ R, const double* __restrict__ AT, int p_first, int NP,
                                                  int KP, int ld, int ci, int cj, int l, double4_t (&acc)[4], double4_t (&dd)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = (double4_t){0.0, 0.0, 0.0, 0.0};
  for (int p0 = p_first; p0 < NP; p0 += 16) {
    double a[4], b[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double* row = R + (size_t)(p0 + 4 * u + (l >> 4)) * ld;
      a[u] = row[ci + (l & 15)];
#pragma unroll
      for (int q = 0; q < 4; ++q) b[u][q] = row[cj + 16 * q + (l & 15)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][q], acc[q], 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) dd[q] = (double4_t){0.0, 0.0, 0.0, 0.0};
  for (int kk = 0; kk < KP; kk += 4) {
    const double* row = AT + (size_t)(kk + (l >> 4)) * ld;
    const double a = row[ci + (l & 15)];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double b = row[cj + 16 * q + (l & 15)];
      dd[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, dd[q], 0, 0, 0);
    }
  }
}

// One work-group per 64 x 64 lower tile (I >= J) of K^-1, wave w owns rows 16w .. 16w+15 of the tile:
//   K^-1[I][J] = sum_{P >= I} R[P][I]^T R[P][J]   (R[P][I] = 0 for P < I),
// i.e. (K^-1)_ij = sum_p R_pi R_pj over the rows p >= 64 I.  A lane's MFMA operands are 16 consecutive columns of one row of R
// (A[i][kk] = R[p0+kk][i], B[kk][j] = R[p0+kk][j]): 128-byte row segments, coalesced.  The epilogue rebuilds the tile's scaled
// distances from AT / nrm with k_gram's MFMA form (the same bits as the Gram the factorisation saw), then reduces
//   W_ij x weight_ij  (i != j, i, j < n)   and, on the diagonal tiles, (K^-1)_ii  (i < n)
// in a fixed order.  Off-diagonal tiles count twice (W and dK are symmetric).  No atomics, no order that depends on the schedule:
// one state, one set of bits.  The two forms of the model (DESIGN.md "GP hyperparameter fit") differ in the weight and in what
// follows it:
//   !ARD  one lengthscale: weight = dK_ij/dlog l (with dist^2 inside), summed per thread, then the wave, then the four waves: S.
//   ARD   one lengthscale per input, folded into the Normalize ranges (k_zstats), so AT holds a_ci = (zn_ci - mean_c) / l_c and the
//         scaled distance, the Gram and K^-1 are the same.  Per input c the fit needs
//           S_c = sum_{i != j} G_ij (a_ci - a_cj)^2,   G_ij = W_ij (5/3) (1 + sqrt5 r_ij) exp(-sqrt5 r_ij),   sum_c S_c = S:
//         the epilogue leaves G in the accumulator layout (0 on the diagonal and for i, j >= n) and then walks the inputs eight at
//         a time: a lane reads its 4 + 4 coordinates of input c and adds its 16 terms in the direct form (the square is not
//         expanded: close points would cancel), wave_sum_multi<8> reduces the eight sums at once, and the four waves are added in
//         wave order through LDS.
// partial[(1 + M) t]: tile t's trace part, then its M sums; M = 1 (S), ARD: M = KP (S_c; rows c >= k of AT are zero).
// k_mll_finish adds them in tile order.
// Batched (pcabo_batch_gp_mll / pcabo_batch_gp_fit and their _ard forms): blockIdx.z = run, every operand zs bytes further per
// run, KP from the run's own k (the runs of a PCA batch differ in k); n and NP are common.  No sum crosses a run, so a run's bits
// are the single launch's.  ARD with M differing per run: run b's partial block starts at its own base (partial + b zs) and is
// packed at ITS stride, 1 + KP_b doubles per tile, exactly as its single launch lays it out; only `out` lies at one offset for
// all runs, which the host puts behind the widest block ((1 + KP_max) tiles doubles in), so one strided copy of 5 + KP_max
// doubles per run brings every run's results back (a narrower run's words beyond 5 + KP_b are never written and never read).
#define MLL_ARD_CHUNK 8
template <bool ARD>
__global__ __launch_bounds__(256) void k_mll_grad(const double* __restrict__ R, const double* __restrict__ AT,
                                                  const double* __restrict__ nrm, const double* __restrict__ alpha, int n,
                                                  int NP, int KP, int ld, double* __restrict__ partial,
                                                  const int* __restrict__ k_dev, size_t zs) {
  ZRUN(R); ZRUN(AT); ZRUN(nrm); ZRUN(alpha); ZRUN(partial); ZRUN(k_dev);
  if (k_dev) KP = (*k_dev + 3) & ~3;
  __shared__ double s_red[4][1 + (ARD ? PCABO_MAXD : 1)];    // per wave: its trace part, then its M sums
  const int t = blockIdx.x;
  const MllTile tile = mll_tile(t);
  const int I = tile.I, J = tile.J;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int ci = I * BS + 16 * w, cj = J * BS;                 // first column of this wave's A rows / of the tile's B columns
  double4_t acc[4], dd[4];
  mll_tile_products(R, AT, I * BS, NP, KP, ld, ci, cj, l, acc, dd);
  const double s5 = 2.23606797749979;   // sqrt(5)
  double sw = 0.0, st = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = cj + 16 * q + (l & 15);                      // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 reg
    const bool jn = j < n;
    const double nj = jn ? nrm[j] : 0.0, aj = jn ? alpha[j] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ci + (l >> 4) + 4 * r;
      const double kinv = acc[q][r];
      double g = 0.0;
      if (i < n && jn) {
        if (i == j) {
          st += kinv;                                          // dK_ii = 0: the diagonal adds to the trace only
        } else {
          double sq = (nrm[i] + nj) - 2.0 * dd[q][r];
          sq = fmax(sq, 0.0);
          const double dist = sqrt(fmax(sq, 1e-30));
          if constexpr (ARD) g = (alpha[i] * aj - kinv) * ((5.0 / 3.0) * (1.0 + s5 * dist) * exp(-s5 * dist));
          else sw += (alpha[i] * aj - kinv) * ((5.0 / 3.0) * (dist * dist) * (1.0 + s5 * dist) * exp(-s5 * dist));
        }
      }
      if constexpr (ARD) acc[q][r] = g;
    }
  }
  if constexpr (!ARD) sw = wave_sum(sw);
  st = wave_sum(st);
  if (l == 0) {
    s_red[w][0] = st;
    if constexpr (!ARD) s_red[w][1] = sw;
  }
  if constexpr (ARD) {
    // (all indices below stay inside the NP columns of AT: ci + 15 < NP, cj + 63 < NP; rows c < KP only)
    for (int c0 = 0; c0 < KP; c0 += MLL_ARD_CHUNK) {
      double v[MLL_ARD_CHUNK];
#pragma unroll
      for (int u = 0; u < MLL_ARD_CHUNK; ++u) {
        v[u] = 0.0;
        if (c0 + u < KP) {                                     // (uniform: KP is a multiple of 4, not of 8)
          const double* row = AT + (size_t)(c0 + u) * ld;
          double ai[4], bj[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) ai[r] = row[ci + (l >> 4) + 4 * r];
#pragma unroll
          for (int q = 0; q < 4; ++q) bj[q] = row[cj + 16 * q + (l & 15)];
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const double d = ai[r] - bj[q];
              s += acc[q][r] * (d * d);
            }
          v[u] = s;
        }
      }
      wave_sum_multi<MLL_ARD_CHUNK>(v, l);
      const int own = wave_multi_owner<MLL_ARD_CHUNK>(l);
      if (own >= 0 && c0 + own < KP) s_red[w][1 + c0 + own] = v[0];
    }
  }
  __syncthreads();
  const int M = ARD ? KP : 1;
  double* out = partial + (size_t)(1 + M) * t;
  const double f = (I == J) ? 1.0 : 2.0;
  if (threadIdx.x <= M) {                                      // thread 0: the trace (every tile counts once), thread 1 + c: sum c
    const int c = threadIdx.x;
    out[c] = (c ? f : 1.0) * (((s_red[0][c] + s_red[1][c]) + s_red[2][c]) + s_red[3][c]);
  }
}

// The results of one evaluation, one work-group, fixed order:
//   out[0] = sum_i log L_ii,  out[1] = y_s^T alpha,  out[2] = sum_i alpha_i,  out[3] = alpha^T alpha,  out[4] = tr K^-1
// strided per thread, then the waves in order (the trace over the tile partials of k_mll_grad), and
//   !ARD  out[5] = S: one more sum of the same kind over the tile partials
//   ARD   out[5 + c] = S_c, c < KP: thread c adds its tile partials in tile order
#define MLL_FIN_THREADS 256
template <bool ARD>
__global__ __launch_bounds__(MLL_FIN_THREADS) void k_mll_finish(const double* __restrict__ L, const double* __restrict__ ys,
                                                               const double* __restrict__ alpha, int n, int ld, int KP,
                                                               const double* __restrict__ partial, int tiles,
                                                               double* __restrict__ out, const int* __restrict__ k_dev, size_t zs) {
  ZRUN(L); ZRUN(ys); ZRUN(alpha); ZRUN(partial); ZRUN(out); ZRUN(k_dev);
  if (k_dev) KP = (*k_dev + 3) & ~3;
  constexpr int NS = ARD ? 5 : 6;                              // the sums reduced over the work-group
  __shared__ double s_red[NS][MLL_FIN_THREADS / 64];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const size_t stride = 1 + (size_t)(ARD ? KP : 1);            // doubles per tile in partial
  double v[NS] = {};
  for (int i = tid; i < n; i += MLL_FIN_THREADS) {
    const double a = alpha[i];
    v[0] += log(L[(size_t)i * ld + i]);
    v[1] += ys[i] * a;
    v[2] += a;
    v[3] += a * a;
  }
  for (int t = tid; t < tiles; t += MLL_FIN_THREADS) {
    v[4] += partial[stride * t];
    if constexpr (!ARD) v[5] += partial[stride * t + 1];
  }
#pragma unroll
  for (int u = 0; u < NS; ++u) {
    const double s = wave_sum(v[u]);
    if (l == 0) s_red[u][w] = s;
  }
  if (ARD && tid < KP) {
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += partial[stride * t + 1 + tid];
    out[5 + tid] = s;
  }
  __syncthreads();
  if (tid < NS) {
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < MLL_FIN_THREADS / 64; ++u) s += s_red[tid][u];
    out[tid] = s;
  }
}

template <bool ARD>
static void launch_mll_form(hipStream_t s, const double* R, const double* AT, const double* nrm, const double* alpha, const double* L,
                            const double* ys, int n, int NP, int KP, int ld, double* partial, double* out, const int* k_dev, ZB zb) {
  const int nb = NP / BS, tiles = nb * (nb + 1) / 2;
  hipLaunchKernelGGL(k_mll_grad<ARD>, dim3(tiles, 1, zb.B), dim3(256), 0, s, R, AT, nrm, alpha, n, NP, KP, ld, partial, k_dev, zb.zs);
  hipLaunchKernelGGL(k_mll_finish<ARD>, dim3(1, 1, zb.B), dim3(MLL_FIN_THREADS), 0, s, L, ys, alpha, n, ld, KP, partial, tiles, out,
                     k_dev, zb.zs);
}
void launch_mll_grad(hipStream_t s, bool ard, const double* R, const double* AT, const double* nrm, const double* alpha,
                     const double* L, const double* ys, int n, int NP, int KP, int ld, double* partial, double* out, const int* k_dev,
                     ZB zb) {
  (ard ? launch_mll_form<true> : launch_mll_form<false>)(s, R, AT, nrm, alpha, L, ys, n, NP, KP, ld, partial, out, k_dev, zb);
}
