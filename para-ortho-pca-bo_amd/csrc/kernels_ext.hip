// Appending points to a conditioned GP and taking them back (pcabo_gp_extend / pcabo_gp_truncate; DESIGN.md "Extending a conditioned
// GP").
//
// The library keeps R = L^-1 explicitly, so one more point borders both factors with two matrix-vector products: with ks = k(xn, Zn),
//   v = R ks (the new row of L),  w = R^T v (= K^-1 ks),  d^2 = (1 + s2 + rung) - |v|^2,
//   L[n] = [v, d],  R[n] = [-w / d, 1 / d].
// Transforms and hyperparameters are held: the Normalize bounds, the Standardize statistics, zn_mean, 1 / lengthscale, the noise and the
// jitter rung are read where the conditioning (or the fit) left them.  Launches per point:
//   k_ext_ks        the point normalised with the held bounds, ks_j for j < n (the direct form of k_score_ks), the partial sums of the
//                   believer mean alpha . ks per 256 points, the standardised value
//   launch_alpha    k_rmatvec / k_rtmatvec unchanged: v = R ks, w = R^T v
//   k_ext_append    d^2 formed and checked by every work-group in the same order (so they agree bit for bit); work-group 0 writes row
//                   n of L and R, column n of ZnT / AT, nrm[n] and ys[n]; when n was a multiple of 64 the other work-groups write the
//                   new padding: identity on the 64 new rows and columns of L and R, zeros in the new columns of ZnT / AT / nrm.
//                   Nothing is written when d^2 fails, except the header's info word (1 + index of the point in the call).
// The header (EXT_HDR doubles in the scratch) is written by the host before the first launch: the rung, and an info word of 0.
// Every kernel here returns at once where the info word is not 0: the points behind a failed one change nothing.
// All sums have one order and there are no atomics: the same call on the same state gives the same bytes.
// The kernels address their operands as the conditioning's do (blockIdx.z = run, zs bytes per run, k from k_dev, 1 / lengthscale
// and the noise from a run's hyperparameter block).  ONE host sequence launches them (ext_append / ext_take_back in pcabo_api.hip, on
// an ExtSite): for a single context - one run, strides 0 - and for all runs of a batch at once, every run with a header of its own.
// A run that takes no part in the call has the info word EXT_INFO_SKIP, written by the host: not 0, so the kernels here (and the
// gated form of launch_alpha between them) leave its bytes alone, and negative, so it is never taken for a failed point.
// The launchers take the arrays a call writes as one record (GpArrays, built by gp_arrays(ctx)), as they take the model as GpModel.
#include "pcabo_internal.h"
#include "acq_math.h"

__device__ inline const int* ext_info(const double* small) { return reinterpret_cast<const int*>(small + EXT_HDR_INFO); }

__global__ __launch_bounds__(256) void k_ext_ks(const double* __restrict__ X, int xi, const double* __restrict__ Y, int yi, int n, int k,
                                                int NP, int ld, const double* __restrict__ ZnT, const double* __restrict__ alpha,
                                                const double* __restrict__ bounds4, const double* __restrict__ ystats, double inv_ls,
                                                int kernel, double* __restrict__ ks, double* __restrict__ small, size_t zs,
                                                const int* __restrict__ k_dev, const double* __restrict__ hyp) {
  ZRUN(X); ZRUN(Y); ZRUN(ZnT); ZRUN(alpha); ZRUN(bounds4); ZRUN(ystats); ZRUN(ks); ZRUN(small);
  if (k_dev) k = *zrun(k_dev, zs, blockIdx.z);
  if (hyp) inv_ls = zrun(hyp, zs, blockIdx.z)[PCABO_HYP_INV_LS];
  if (*ext_info(small) != 0) return;
  __shared__ double s_xn[PCABO_MAXD];
  __shared__ double s_mu[4];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const double* x = X + (size_t)xi * k;
  if (tid < k) {
    const double lo = bounds4[tid], hi = bounds4[PCABO_MAXD + tid];
    s_xn[tid] = (x[tid] - lo) / (hi - lo);
  }
  __syncthreads();
  const int j = blockIdx.x * 256 + tid;
  double sq = 0.0;
  if (j < n) {
    for (int c0 = 0; c0 < k; c0 += 8) {                // eight loads in flight; the sum keeps its order
      double z[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) z[u] = (c0 + u < k) ? ZnT[(size_t)(c0 + u) * ld + j] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c0 + u < k) { const double d = s_xn[c0 + u] - z[u]; sq += d * d; }
    }
  }
  const double kv = j < n ? acq_cov_value(sq * (inv_ls * inv_ls), kernel) : 0.0;
  if (j < NP) ks[j] = kv;
  const double m = wave_sum((j < n ? alpha[j] : 0.0) * kv);
  if (l == 0) s_mu[w] = m;
  __syncthreads();
  if (tid == 0) small[EXT_MU + blockIdx.x] = ((s_mu[0] + s_mu[1]) + s_mu[2]) + s_mu[3];
  if (blockIdx.x == 0) {
    if (tid < k) small[EXT_XN + tid] = s_xn[tid];
    if (tid == 0 && Y) small[EXT_YS] = (Y[yi] - ystats[0]) / ystats[1];
  }
}

// grid (1, 1, B), or (1 + NPnew / 64, 1, B) when the point opens a new 64-block (n == NP): work-group 1 + cb then owns the column
// chunk cb of the new rows and, for cb < NP / 64, the block above the diagonal in the new columns.
__global__ __launch_bounds__(256) void k_ext_append(const double* __restrict__ v, const double* __restrict__ wv,
                                                    double* __restrict__ small, int idx, int believer, int njb, int n, int k, int NP,
                                                    int ld, double s2, double inv_ls, const double* __restrict__ zn_mean,
                                                    double* __restrict__ L, double* __restrict__ R, double* __restrict__ ZnT,
                                                    double* __restrict__ AT, double* __restrict__ nrm, double* __restrict__ ys,
                                                    size_t zs, const int* __restrict__ k_dev, const double* __restrict__ hyp) {
  ZRUN(v); ZRUN(wv); ZRUN(small); ZRUN(zn_mean); ZRUN(L); ZRUN(R); ZRUN(ZnT); ZRUN(AT); ZRUN(nrm); ZRUN(ys);
  if (k_dev) k = *zrun(k_dev, zs, blockIdx.z);
  if (hyp) { inv_ls = zrun(hyp, zs, blockIdx.z)[PCABO_HYP_INV_LS]; s2 = zrun(hyp, zs, blockIdx.z)[PCABO_HYP_NOISE]; }
  __shared__ double s_red[4];
  __shared__ double s_a[PCABO_MAXD];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  // (read before any work-group of this launch can have written it: the word is only ever set from 0, by work-group 0, where
  //  every work-group finds the same d^2 and writes nothing anyway)
  if (*ext_info(small) != 0) return;
  double acc = 0.0;
  for (int p = tid; p < n; p += 256) { const double x = v[p]; acc = fma(x, x, acc); }
  acc = wave_sum(acc);
  if (l == 0) s_red[w] = acc;
  __syncthreads();
  const double vv = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
  const double d2 = ((1.0 + s2) + small[EXT_HDR_RUNG]) - vv;
  if (!(d2 > 0.0) || !(d2 <= 1.7976931348623157e308)) {
    if (blockIdx.x == 0 && tid == 0) *reinterpret_cast<int*>(small + EXT_HDR_INFO) = 1 + idx;
    return;
  }
  const bool grow = n == NP;
  const int NPn = grow ? NP + 64 : NP, KP = (k + 3) & ~3;
  if (blockIdx.x == 0) {
    const double d = sqrt(d2);
    double* Lr = L + (size_t)n * ld;
    double* Rr = R + (size_t)n * ld;
    for (int j = tid; j < NPn; j += 256) {
      double lv = 0.0, rv = 0.0;
      if (j < n) { lv = v[j]; rv = -wv[j] / d; }
      else if (j == n) { lv = d; rv = 1.0 / d; }
      else if (!grow) continue;                        // (the padding of the current block: zeros already)
      Lr[j] = lv; Rr[j] = rv;
    }
    if (tid < KP) {
      double xn = 0.0, a = 0.0;
      if (tid < k) { xn = small[EXT_XN + tid]; a = (xn - zn_mean[tid]) * inv_ls; }
      ZnT[(size_t)tid * ld + n] = xn;
      AT[(size_t)tid * ld + n] = a;
      s_a[tid] = a;
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int c = 0; c < KP; ++c) s += s_a[c] * s_a[c];
      nrm[n] = s;
      double y = small[EXT_YS];
      if (believer) {
        y = 0.0;
        for (int b = 0; b < njb; ++b) y += small[EXT_MU + b];
      }
      ys[n] = y;
    }
    return;
  }
  // the new padding (grow only): nothing may be assumed about what the capacity buffers held there
  const int cb = blockIdx.x - 1, c0 = cb * 64;
  for (int idx2 = tid; idx2 < 63 * 64; idx2 += 256) {
    const int r = n + 1 + (idx2 >> 6), c = c0 + (idx2 & 63);
    const double e = r == c ? 1.0 : 0.0;
    L[(size_t)r * ld + c] = e;
    R[(size_t)r * ld + c] = e;
  }
  if (c0 < NP) {
    for (int idx2 = tid; idx2 < 64 * 64; idx2 += 256) {
      const int r = c0 + (idx2 >> 6), c = NP + (idx2 & 63);
      L[(size_t)r * ld + c] = 0.0;
      R[(size_t)r * ld + c] = 0.0;
    }
  } else {
    // the last work-group (the new diagonal block): the new columns of ZnT / AT / nrm behind the point itself
    for (int idx2 = tid; idx2 < KP * 64; idx2 += 256) {
      const int c = idx2 >> 6, j = NP + (idx2 & 63);
      if (j == n) continue;
      ZnT[(size_t)c * ld + j] = 0.0;
      AT[(size_t)c * ld + j] = 0.0;
    }
    if (tid >= 1 && tid < 64) nrm[NP + tid] = 0.0;
  }
}

// Points n0 .. are taken back: the identity on rows n0 .. NP - 1 of L and R (work-group cb: the column chunk cb), zeros in columns
// n0 .. NP - 1 of ZnT / AT and in nrm / ys there (the last work-group).  NP: the padded size before the call.  grid (NP / 64, 1, B).
__global__ __launch_bounds__(256) void k_ext_truncate(const double* __restrict__ small, int n0, int k, int NP, int ld,
                                                      double* __restrict__ L, double* __restrict__ R, double* __restrict__ ZnT,
                                                      double* __restrict__ AT, double* __restrict__ nrm, double* __restrict__ ys,
                                                      size_t zs, const int* __restrict__ k_dev) {
  ZRUN(small); ZRUN(L); ZRUN(R); ZRUN(ZnT); ZRUN(AT); ZRUN(nrm); ZRUN(ys);
  if (k_dev) k = *zrun(k_dev, zs, blockIdx.z);
  if (*ext_info(small) != 0) return;
  const int tid = threadIdx.x, c = blockIdx.x * 64 + (tid & 63);
  for (int r = n0 + (tid >> 6); r < NP; r += 4) {
    const double e = r == c ? 1.0 : 0.0;
    L[(size_t)r * ld + c] = e;
    R[(size_t)r * ld + c] = e;
  }
  if (blockIdx.x != gridDim.x - 1) return;
  const int KP = (k + 3) & ~3, m = NP - n0;
  for (int idx = tid; idx < KP * m; idx += 256) {
    const int cc = idx / m, j = n0 + (idx - cc * m);
    ZnT[(size_t)cc * ld + j] = 0.0;
    AT[(size_t)cc * ld + j] = 0.0;
  }
  for (int j = n0 + tid; j < NP; j += 256) { nrm[j] = 0.0; ys[j] = 0.0; }
}

void launch_ext_ks(hipStream_t st, const double* X, int xi, const double* Y, int yi, const GpModel& m, double inv_ls, int kernel,
                   const ExtScratch& e, AcqBatch ab, int B) {
  hipLaunchKernelGGL(k_ext_ks, dim3((m.NP + 255) / 256, 1, B), dim3(256), 0, st, X, xi, Y, yi, m.n, m.k, m.NP, m.ld, m.ZnT, m.alpha,
                     m.bounds4, m.ystats, inv_ls, kernel, e.ks, e.small, ab.zs, ab.k_dev, ab.hyp);
}
void launch_ext_append(hipStream_t st, const GpModel& m, const ExtScratch& e, int idx, int believer, double s2, double inv_ls,
                       const GpArrays& a, AcqBatch ab, int B) {
  const int groups = m.n == m.NP ? 1 + (m.NP + 64) / 64 : 1;
  hipLaunchKernelGGL(k_ext_append, dim3(groups, 1, B), dim3(256), 0, st, e.v, e.w, e.small, idx, believer, (m.NP + 255) / 256, m.n, m.k,
                     m.NP, m.ld, s2, inv_ls, a.zn_mean, a.L, a.R, a.ZnT, a.AT, a.nrm, a.ys, ab.zs, ab.k_dev, ab.hyp);
}
void launch_ext_truncate(hipStream_t st, const ExtScratch& e, int n0, int k, int NP, int ld, const GpArrays& a, AcqBatch ab, int B) {
  hipLaunchKernelGGL(k_ext_truncate, dim3(NP / 64, 1, B), dim3(256), 0, st, e.small, n0, k, NP, ld, a.L, a.R, a.ZnT, a.AT, a.nrm, a.ys,
                     ab.zs, ab.k_dev);
}
