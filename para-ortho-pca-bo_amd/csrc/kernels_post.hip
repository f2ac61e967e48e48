// Posterior of the conditioned GP at q query points of the reduced space: mean, variance and joint covariance
// (pcabo_gp_posterior / pcabo_batch_gp_posterior; DESIGN.md "GP posterior queries").
//
// gpytorch's model.posterior(X) for SingleTaskGP(MaternKernel | RBFKernel, Standardize, Normalize) without an output scale, from the
// state the conditioning kernels left (ZnT, R = L^-1, alpha, Standardize statistics):
//   ks = k(xn, Zn),  V = R KS^T (NP x q)
//   mean_a  = m_y + s_y sum_j alpha_j ks_aj
//   var_a   = s_y^2 (1 [+ s2] - |v_a|^2), floored at 1e-10 (gpytorch's min_variance)
//   cov_ab  = s_y^2 (k(xn_a, xn_b) [+ s2 delta_ab] - v_a . v_b), not floored
// The launches are those of the value-only scoring (kernels_acq.hip) up to the scalar chain:
//   k_score_ks      KS and the mu_s records, unchanged
//   k_score_gemm    the scoring's own kernel (launch_score_gemm), with a covariance asked for in the instantiation that also stores
//                   V: one tile product and one column-norm epilogue, so |v|^2 has the scoring's bits because it is the same code
//   k_post_combine  one wave per query: the S records added in acq_finish_query's order, then mean and variance instead of an
//                   acquisition value; the variance before the floor is kept for the covariance's diagonal
//   k_post_cov      V^T V per lower 64 x 64 tile through the shared tile product (tile_product_f64, pcabo_internal.h; K-major
//                   operands), the prior part rebuilt from the normalised queries in the epilogue, tile and mirror written by the one
//                   work-group that owns them: no atomics, the same bits on every call
// Batches: blockIdx.z = run, zrun addressing, k of a run from k_dev, 1 / lengthscale and the noise from its hyperparameter block.
//
// Joint samples (pcabo_gp_posterior_sample / pcabo_batch_gp_posterior_sample; DESIGN.md "GP posterior samples") go on behind the
// covariance:
//   k_post_chol_prep  cov + j s_y^2 I into the padded factor buffer (identity on the padding), the Cholesky's info word cleared
//   launch_cholesky   the GP's own blocked factorisation, in place (kernels_gp.hip / kernels_gpw.hip), unchanged
//   k_post_sample     out = [mean +] base Lc^T per 64 x 64 tile through tile_product_f64, the column blocks of Lc in ascending order
//
// Leave-one-out predictions at the data themselves (pcabo_gp_loo / pcabo_batch_gp_loo; DESIGN.md "Leave-one-out predictions") need
// no query: k_loo reads the lower triangle of R once and runs a scalar chain per point.
#include "pcabo_internal.h"
#include "acq_math.h"

// One wave per query: out[q] = mean, out[q_total + q] = variance (floored), out[2 q_total + q] = the variance before the floor.
__global__ __launch_bounds__(256) void k_post_combine(const double* __restrict__ partial, int q_total, int S,
                                                      const double* __restrict__ ystats, double s2, int obs_noise,
                                                      double* __restrict__ out, size_t zs, const double* __restrict__ hyp) {
  ZRUN(partial); ZRUN(ystats); ZRUN(out);
  if (hyp) s2 = zrun(hyp, zs, blockIdx.z)[PCABO_HYP_NOISE];
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (q >= q_total) return;
  const double* base = partial + (size_t)q * S * PCABO_PSTRIDE;
  const double ym = ystats[0], ysd = ystats[1];
  double vv = 0.0, mus = 0.0;
  for (int s = l; s < S; s += 64) { vv += base[(size_t)s * PCABO_PSTRIDE]; mus += base[(size_t)s * PCABO_PSTRIDE + 1]; }
  vv = wave_sum(vv);
  mus = wave_sum(mus);
  const double mu = ym + ysd * mus;
  double var = obs_noise ? ((1.0 - vv) + s2) * (ysd * ysd) : (1.0 - vv) * (ysd * ysd);
  const double raw = var;
  if (!(var >= 1e-10)) var = 1e-10;          // gpytorch min_variance (double)
  if (l == 0) {
    out[q] = mu;
    out[(size_t)q_total + q] = var;
    out[2 * (size_t)q_total + q] = raw;
  }
}

// cov = s_y^2 (k(Xq, Xq) - V^T V) off the diagonal, the combine pass' unfloored variance on it.  Work-group t owns the lower tile
// (A, Bt), A >= Bt, and writes it and its mirror.
__global__ __launch_bounds__(256) void k_post_cov(const double* __restrict__ V, int q_total, int NP, const double* __restrict__ Xq,
                                                  int k, const double* __restrict__ bounds4, const double* __restrict__ ystats,
                                                  const double* __restrict__ raw_var, double inv_ls, int kernel,
                                                  double* __restrict__ cov, size_t zs, size_t vzs, const int* __restrict__ k_dev,
                                                  const double* __restrict__ hyp) {
  ZRUN(Xq); ZRUN(bounds4); ZRUN(ystats); ZRUN(raw_var);
  V = zrun(V, vzs, blockIdx.z); cov = zrun(cov, vzs, blockIdx.z);
  if (k_dev) k = *zrun(k_dev, zs, blockIdx.z);
  if (hyp) inv_ls = zrun(hyp, zs, blockIdx.z)[PCABO_HYP_INV_LS];
  __shared__ __attribute__((aligned(16))) double s_a[64 * PCABO_TLD];
  __shared__ __attribute__((aligned(16))) double s_b[64 * PCABO_TLD];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  int A = 0, Bt = blockIdx.x;
  while (Bt > A) { Bt -= A + 1; ++A; }       // lower tiles row by row: (0,0) (1,0) (1,1) (2,0) ...
  const size_t Q = (size_t)q_total;
  double4_t acc[4];
  // rows 64 P .. of V, ascending: the columns of tile A and of tile Bt (zeros beyond q).  The tiles lie [row of V][query]
  tile_product_f64<true>(s_a, s_b, NP / 64, [&](int P, int r, int c, double& a, double& b) {
    const double* row = V + (size_t)(P * 64 + r) * Q;
    a = (A * 64 + c < q_total) ? row[A * 64 + c] : 0.0;
    b = (Bt * 64 + c < q_total) ? row[Bt * 64 + c] : 0.0;
  }, acc);
  // acc[t][r] = (V^T V)[64 A + 16 w + (l >> 4) + 4 r][64 Bt + 16 t + (l & 15)].  The prior part: squared distances of the
  // normalised queries in the direct form, 64 coordinates at a time through the two tiles (query, coordinate), ascending.
  double sq[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) sq[t][r] = 0.0;
  for (int c0 = 0; c0 < k; c0 += 64) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int idx = tid + 256 * u, r = idx >> 6, c = idx & 63;
      double xa = 0.0, xb = 0.0;
      if (c0 + c < k) {
        const double lo = bounds4[c0 + c], hi = bounds4[PCABO_MAXD + c0 + c];
        if (A * 64 + r < q_total) xa = (Xq[(size_t)(A * 64 + r) * k + c0 + c] - lo) / (hi - lo);
        if (Bt * 64 + r < q_total) xb = (Xq[(size_t)(Bt * 64 + r) * k + c0 + c] - lo) / (hi - lo);
      }
      s_a[r * PCABO_TLD + c] = xa;
      s_b[r * PCABO_TLD + c] = xb;
    }
    __syncthreads();
    const int cn = k - c0 < 64 ? k - c0 : 64;
    for (int c = 0; c < cn; ++c) {
      double xa[4], xb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) xa[r] = s_a[(16 * w + (l >> 4) + 4 * r) * PCABO_TLD + c];
#pragma unroll
      for (int t = 0; t < 4; ++t) xb[t] = s_b[(16 * t + (l & 15)) * PCABO_TLD + c];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const double d = xa[r] - xb[t]; sq[t][r] += d * d; }
    }
  }
  const double ysd = ystats[1], sy2 = ysd * ysd;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = 16 * t + (l & 15);
    const size_t b = (size_t)Bt * 64 + j;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * w + (l >> 4) + 4 * r;
      const size_t a = (size_t)A * 64 + i;
      if (a >= Q || b >= Q) continue;
      if (a == b) { cov[a * Q + a] = raw_var[a]; continue; }
      if (A == Bt && i < j) continue;          // a diagonal tile: its upper half is the mirror of its lower half
      const double c = (acq_cov_value(sq[t][r] * (inv_ls * inv_ls), kernel) - acc[t][r]) * sy2;
      cov[a * Q + b] = c;
      cov[b * Q + a] = c;
    }
  }
}

// The whole query: KS and the mu_s records (the scoring's first launch), V = R KS^T with its column norms, mean and variance per query
// into post[3 q] and, with V / cov given, the q x q covariance.  B > 1: the runs of a batch (strides zs; vzs between their V / cov).
void launch_posterior(hipStream_t st, const double* Xq, int q, const GpModel& m, AcqParams p, double s2, int obs_noise,
                      double* KS, double* partial, double* post, double* V, double* cov, AcqBatch ab, size_t vzs, int B) {
  const int S = m.NP / 64;
  launch_score_ks(st, Xq, q, m, p, KS, partial, ab, B);
  launch_score_gemm(st, m, q, KS, partial, ab.zs, B, V, vzs);
  hipLaunchKernelGGL(k_post_combine, dim3((q + 3) / 4, 1, B), dim3(256), 0, st, partial, q, S, m.ystats, s2, obs_noise, post, ab.zs,
                     ab.hyp);
  if (!cov) return;
  const int nt = (q + 63) / 64;
  hipLaunchKernelGGL(k_post_cov, dim3(nt * (nt + 1) / 2, 1, B), dim3(256), 0, st, V, q, m.NP, Xq, m.k, m.bounds4, m.ystats,
                     post + 2 * (size_t)q, p.inv_ls, p.kernel, cov, ab.zs, vzs, ab.k_dev, ab.hyp);
}

// ---- joint samples --------------------------------------------------------------------------------------------------------------
// F (QP x QP, ld = QP, QP = 64 ceil(q / 64)) = cov + jitter s_y^2 I on the leading q x q part, the identity on the padding rows and
// columns; one work-group per 64 x 64 tile.  The whole square is written, so a retry on the next rung starts from the untouched cov.
// szs: bytes between two runs' sample blocks (F and info), vzs: between their cov blocks.
__global__ __launch_bounds__(256) void k_post_chol_prep(const double* __restrict__ cov, int q_total, int QP,
                                                        const double* __restrict__ ystats, double jitter, double* __restrict__ F,
                                                        int* __restrict__ info, size_t zs, size_t vzs, size_t szs) {
  ZRUN(ystats);
  cov = zrun(cov, vzs, blockIdx.z); F = zrun(F, szs, blockIdx.z); info = zrun(info, szs, blockIdx.z);
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *info = 0;
  const double ysd = ystats[1], add = jitter * (ysd * ysd);
  const size_t Q = (size_t)q_total;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int idx = tid + 256 * u;
    const int a = blockIdx.y * 64 + (idx >> 6), b = blockIdx.x * 64 + (idx & 63);
    double v;
    if (a < q_total && b < q_total) {
      v = cov[a * Q + b];
      if (a == b) v += add;
    } else {
      v = (a == b) ? 1.0 : 0.0;
    }
    F[(size_t)a * QP + b] = v;
  }
}

// out[s][a] = [mean_a +] sum_{b <= a} Lc[a][b] base[s][b]: work-group (x, y) owns samples 64 x .. and points 64 y .. and walks the
// column blocks J <= y of Lc.  Lc is the factored F: below the diagonal the factor, ABOVE it whatever the input held (the Cholesky
// never writes there), so the diagonal tile is masked to its lower half; rows and columns >= q (the identity padding) and samples
// >= S are staged as zeros and never stored.  base and out: S x q dense.  mean: null for the centred process.
__global__ __launch_bounds__(256) void k_post_sample(const double* __restrict__ F, int q_total, int QP, const double* __restrict__ base,
                                                     int S, const double* __restrict__ mean, double* __restrict__ out, size_t zs,
                                                     size_t szs) {
  ZRUN(mean);
  F = zrun(F, szs, blockIdx.z); base = zrun(base, szs, blockIdx.z); out = zrun(out, szs, blockIdx.z);
  __shared__ __attribute__((aligned(16))) double s_a[64 * PCABO_TLD];
  __shared__ __attribute__((aligned(16))) double s_b[64 * PCABO_TLD];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int s0 = blockIdx.x * 64, A = blockIdx.y;
  const size_t Q = (size_t)q_total;
  double4_t acc[4];
  // ascending column blocks J <= A: base rows s0 .., columns 64 J ..; Lc rows 64 A .., columns 64 J ..
  tile_product_f64<false>(s_a, s_b, A + 1, [&](int J, int r, int c, double& pa, double& pb) {
    const int b = J * 64 + c, a = A * 64 + r;
    pa = (s0 + r < S && b < q_total) ? base[(size_t)(s0 + r) * Q + b] : 0.0;
    pb = (a < q_total && b <= a) ? F[(size_t)a * QP + b] : 0.0;      // (b <= a < q: the lower triangle of the q x q part)
  }, acc);
  // acc[t][r] = (base Lc^T)[s0 + 16 w + (l >> 4) + 4 r][64 A + 16 t + (l & 15)]
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int a = A * 64 + 16 * t + (l & 15);
    if (a >= q_total) continue;
    const double m = mean ? mean[a] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = s0 + 16 * w + (l >> 4) + 4 * r;
      if (s < S) out[(size_t)s * Q + a] = mean ? m + acc[t][r] : acc[t][r];
    }
  }
}

// ---- leave-one-out predictions (pcabo_gp_loo / pcabo_batch_gp_loo; DESIGN.md "Leave-one-out predictions") ------------------------
// For every observed point i < n, from R = L^-1, alpha, y_s and (m', s) as the conditioning left them (include/pcabo.h):
//   d_i = sum_{p >= i} R[p][i]^2 = (K^-1)_ii,  r_i = alpha_i / d_i,  mean_i = m' + s (ys_i - r_i),  var_i = s^2 / d_i,
//   z_i = r_i sqrt(d_i),  lpd_i = -1/2 (log 2 pi + log var_i + z_i^2);   out = mean | var | z | lpd, n doubles each.
// One work-group per 64-column block J, lane = column: a row segment of R is one coalesced 512-byte read.  Wave w walks the rows
// 64 J + w, + 4, ... < n in ascending order, LOO_ROWS of them in flight per trip, and adds their squares one after the other into
// ONE accumulator; the four waves' sums are then added in wave order through LDS and wave 0 runs the scalar chain of its 64
// columns.  Every sum has one order that no schedule changes: the same state gives the same bits on every call.  Entries above the
// diagonal are masked (the definition's p >= i), rows >= n (the identity padding) are never read.
// Batched: blockIdx.z = run, every operand zs bytes further per run; n and NP are common.  No sum crosses a run.
#define LOO_ROWS 8
__global__ __launch_bounds__(256) void k_loo(const double* __restrict__ R, const double* __restrict__ alpha,
                                             const double* __restrict__ ys, const double* __restrict__ ystats, int n, int ld,
                                             double* __restrict__ out, size_t zs) {
  ZRUN(R); ZRUN(alpha); ZRUN(ys); ZRUN(ystats); ZRUN(out);
  __shared__ double s_d[4][64];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int c = blockIdx.x * 64 + l;              // (c < NP <= ld: inside the row also where c >= n)
  const double* col = R + c;
  double d = 0.0;
  int p = blockIdx.x * 64 + w;
  for (; p + 4 * (LOO_ROWS - 1) < n; p += 4 * LOO_ROWS) {
    double v[LOO_ROWS];
#pragma unroll
    for (int u = 0; u < LOO_ROWS; ++u) v[u] = col[(size_t)(p + 4 * u) * ld];
#pragma unroll
    for (int u = 0; u < LOO_ROWS; ++u) { const double x = p + 4 * u >= c ? v[u] : 0.0; d = fma(x, x, d); }
  }
  for (; p < n; p += 4) { const double x = p >= c ? col[(size_t)p * ld] : 0.0; d = fma(x, x, d); }
  s_d[w][l] = d;
  __syncthreads();
  if (w != 0 || c >= n) return;
  d = ((s_d[0][l] + s_d[1][l]) + s_d[2][l]) + s_d[3][l];
  const double m = ystats[0], s = ystats[1];
  const double r = alpha[c] / d;
  const double var = (s * s) / d;
  const double z = r * sqrt(d);
  const size_t N = (size_t)n;
  out[c] = m + s * (ys[c] - r);
  out[N + c] = var;
  out[2 * N + c] = z;
  out[3 * N + c] = -0.5 * ((1.8378770664093453 + log(var)) + z * z);      // log(2 pi)
}

void launch_loo(hipStream_t st, const double* R, const double* alpha, const double* ys, const double* ystats, int n, int ld,
                double* out, size_t zs, int B) {
  hipLaunchKernelGGL(k_loo, dim3((n + 63) / 64, 1, B), dim3(256), 0, st, R, alpha, ys, ystats, n, ld, out, zs);
}

void launch_post_chol_prep(hipStream_t st, const double* cov, int q, const double* ystats, double jitter, double* F, int* info,
                           size_t zs, size_t vzs, size_t szs, int B) {
  const int nb = (q + 63) / 64;
  hipLaunchKernelGGL(k_post_chol_prep, dim3(nb, nb, B), dim3(256), 0, st, cov, q, nb * 64, ystats, jitter, F, info, zs, vzs, szs);
}
void launch_post_sample(hipStream_t st, const double* F, int q, const double* base, int S, const double* mean, double* out, size_t zs,
                        size_t szs, int B) {
  const int nb = (q + 63) / 64;
  hipLaunchKernelGGL(k_post_sample, dim3((S + 63) / 64, nb, B), dim3(256), 0, st, F, q, nb * 64, base, S, mean, out, zs, szs);
}
