// BBOB f15-f24 objective evaluation on gfx950 for the batched multi-run driver.
//
// The reference takes its objectives from the third-party `ioh` package (/root/reference/Algorithms/Experiment/
// ExperimentRunner.py:90, evaluated at PCA_BO.py:263) - one point per BO iteration and run, on the host.  When B runs
// advance in lock-step their B candidates are evaluated here in one launch: one work-group per run, the run's seeded
// tables (x_opt, rotations, conditioning, Gallagher peaks) resident in device memory.  The tables are generated on the
// host by pcabo.bbob (the legacy generators are sequential integer recurrences) and uploaded once per run; the
// arithmetic below follows pcabo.bbob function by function (f15 / f20 pinned by the reference's own data there, the
// others restated from the published definitions: parity unpinned).  Also applies PCA_BO's out-of-box rule
// (PCA_BO.py:248-263): a candidate outside [lb, ub] is not evaluated and gets the penalty value.
#include "../../include/pcabo.h"
#include "pcabo_internal.h"
#include <new>
#include <cstdio>
#include <cstring>

#define BB_THREADS 256
#define BB_PEAKS 101

struct BbobLayout { int d, off_xopt, off_r, off_m, off_aux, stride; };
static BbobLayout bbob_layout(int d) {
  BbobLayout L;
  L.d = d; L.off_xopt = 0; L.off_r = d; L.off_m = d + d * d; L.off_aux = d + 2 * d * d;
  L.stride = L.off_aux + BB_PEAKS * (2 * d + 1) + 4 * d + 8;
  return L;
}

__device__ inline double bb_block_sum(double v, double* s_red) {       // fixed-order tree: deterministic
  const int tid = threadIdx.x;
  s_red[tid] = v;
  __syncthreads();
  for (int off = BB_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) s_red[tid] += s_red[tid + off];
    __syncthreads();
  }
  const double r = s_red[0];
  __syncthreads();
  return r;
}
__device__ inline double bb_block_max(double v, double* s_red) {
  const int tid = threadIdx.x;
  s_red[tid] = v;
  __syncthreads();
  for (int off = BB_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) s_red[tid] = fmax(s_red[tid], s_red[tid + off]);
    __syncthreads();
  }
  const double r = s_red[0];
  __syncthreads();
  return r;
}
__device__ inline double bb_osz(double x) {
  if (x > 0.0) { const double t = log(x) / 0.1; return pow(exp(t + 0.49 * (sin(t) + sin(0.79 * t))), 0.1); }
  if (x < 0.0) { const double t = log(-x) / 0.1; return -pow(exp(t + 0.49 * (sin(0.55 * t) + sin(0.31 * t))), 0.1); }
  return 0.0;
}
__device__ inline double bb_asy(double x, double beta, int i, int d) {
  return x > 0.0 ? pow(x, 1.0 + beta * ((double)i / (d - 1.0)) * sqrt(x)) : x;
}
// out[i] = sum_j A[i][j] v[j] for i < d (A row-major d x d); one thread per row, v in LDS
__device__ inline void bb_matvec(const double* __restrict__ A, const double* v, double* out, int d) {
  for (int i = threadIdx.x; i < d; i += BB_THREADS) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) s += A[(size_t)i * d + j] * v[j];
    out[i] = s;
  }
  __syncthreads();
}

// One candidate of run b by one work-group: its d coordinates at X + row * d, its value and flag written to slot `slot` of raw / oob.
// Both kernels below are this body; the LDS arrays are the work-group's own.
__device__ __forceinline__ void bb_eval_one(const double* __restrict__ tables, const int* __restrict__ fids, const BbobLayout L,
                                            const double* __restrict__ X, const int b, const size_t row, const size_t slot,
                                            const double lb, const double ub, const double penalty, double* __restrict__ raw,
                                            int* __restrict__ oob) {
  __shared__ double s_red[BB_THREADS];
  __shared__ double s_x[PCABO_MAXD], s_a[PCABO_MAXD], s_b[PCABO_MAXD];
  const int tid = threadIdx.x, d = L.d;
  const double* T = tables + (size_t)b * L.stride;
  const double *xopt = T + L.off_xopt, *R = T + L.off_r, *M = T + L.off_m, *aux = T + L.off_aux;
  const int fid = fids[b];
  const double two_pi = 6.283185307179586;
  double pen_loc = 0.0, out_loc = 0.0;
  for (int i = tid; i < d; i += BB_THREADS) {
    const double x = X[row * d + i];
    s_x[i] = x;
    const double o = fabs(x) - 5.0;
    if (o > 0.0) pen_loc += o * o;
    if (!(x >= lb) || !(x <= ub)) out_loc = 1.0;
  }
  __syncthreads();
  const double pen = bb_block_sum(pen_loc, s_red);
  const bool outside = bb_block_sum(out_loc, s_red) > 0.0;
  if (outside) {                             // PCA_BO.py:260-261: not evaluated, fixed penalty
    if (tid == 0) { raw[slot] = penalty; oob[slot] = 1; }
    return;
  }
  double f = 0.0;
  if (fid == 15 || fid == 16 || fid == 17 || fid == 18 || fid == 23) {
    for (int i = tid; i < d; i += BB_THREADS) s_a[i] = s_x[i] - xopt[i];
    __syncthreads();
    if (fid == 23) {
      bb_matvec(M, s_a, s_b, d);                                          // z = M (x - x_opt)
      double lp = 0.0;                                                     // log of the product, summed deterministically
      for (int i = tid; i < d; i += BB_THREADS) {
        double s = 0.0, p2 = 1.0;
        for (int j = 1; j <= 32; ++j) { p2 *= 2.0; const double t = p2 * s_b[i]; s += fabs(t - floor(t + 0.5)) / p2; }
        lp += (10.0 / pow((double)d, 1.2)) * log(1.0 + (i + 1.0) * s);
      }
      const double prod = exp(bb_block_sum(lp, s_red));
      f = 10.0 / d / d * (prod - 1.0) + pen;
    } else {
      bb_matvec(R, s_a, s_b, d);                                          // y = R (x - x_opt)
      for (int i = tid; i < d; i += BB_THREADS) {
        const double y = s_b[i];
        s_a[i] = fid == 15 ? bb_asy(bb_osz(y), 0.2, i, d) : (fid == 16 ? bb_osz(y) : bb_asy(y, 0.5, i, d));
      }
      __syncthreads();
      bb_matvec(M, s_a, s_b, d);                                          // z
      if (fid == 15) {
        double c = 0.0, q = 0.0;
        for (int i = tid; i < d; i += BB_THREADS) { c += cos(two_pi * s_b[i]); q += s_b[i] * s_b[i]; }
        f = 10.0 * (d - bb_block_sum(c, s_red)) + bb_block_sum(q, s_red);
      } else if (fid == 16) {
        double f0 = 0.0, ak = 1.0, bk = 1.0;
        for (int kk = 0; kk < 12; ++kk) { f0 += ak * cos(two_pi * bk * 0.5); ak *= 0.5; bk *= 3.0; }
        double s = 0.0;
        for (int i = tid; i < d; i += BB_THREADS) {
          ak = 1.0; bk = 1.0;
          for (int kk = 0; kk < 12; ++kk) { s += cos(two_pi * (s_b[i] + 0.5) * bk) * ak; ak *= 0.5; bk *= 3.0; }
        }
        const double t = bb_block_sum(s, s_red) / d - f0;
        f = 10.0 * t * t * t + (10.0 / d) * pen;
      } else {
        double s = 0.0;
        for (int i = tid; i < d - 1; i += BB_THREADS) {
          const double t = s_b[i] * s_b[i] + s_b[i + 1] * s_b[i + 1];
          const double sn = sin(50.0 * pow(t, 0.1));
          s += pow(t, 0.25) * (1.0 + sn * sn);
        }
        const double t = bb_block_sum(s, s_red) / (d - 1.0);
        f = t * t + 10.0 * pen;
      }
    }
  } else if (fid == 19) {
    bb_matvec(M, s_x, s_b, d);
    double s = 0.0;
    for (int i = tid; i < d - 1; i += BB_THREADS) {
      const double z0 = s_b[i] + 0.5, z1 = s_b[i + 1] + 0.5;
      const double c1 = z0 * z0 - z1, c2 = 1.0 - z0, t = 100.0 * c1 * c1 + c2 * c2;
      s += t / 4000.0 - cos(t);
    }
    f = 10.0 + 10.0 * bb_block_sum(s, s_red) / (d - 1.0);
  } else if (fid == 20) {
    const double *sign = aux, *offset = aux + d, *cond = aux + 2 * d;
    for (int i = tid; i < d; i += BB_THREADS) s_a[i] = 2.0 * sign[i] * s_x[i];
    __syncthreads();
    double p2 = 0.0, tot = 0.0;
    for (int i = tid; i < d; i += BB_THREADS) {
      double zh = s_a[i];
      if (i > 0) zh += 0.25 * (s_a[i - 1] - offset[i - 1]);
      const double z = 100.0 * (cond[i] * (zh - offset[i]) + offset[i]);
      const double o = fabs(z) - 500.0;
      if (o > 0.0) p2 += o * o;
      tot += z * sin(sqrt(fabs(z)));
    }
    f = 0.01 * (bb_block_sum(p2, s_red) + 418.9828872724339 - bb_block_sum(tot, s_red) / d);
  } else if (fid == 21 || fid == 22) {
    const int P = fid == 21 ? 101 : 21;
    const double *heights = aux, *scales = aux + BB_PEAKS, *centres = aux + BB_PEAKS + BB_PEAKS * d;
    bb_matvec(R, s_x, s_b, d);                                            // tx = R x
    double best = 0.0;
    for (int p = tid; p < P; p += BB_THREADS) {
      double e = 0.0;
      for (int j = 0; j < d; ++j) { const double df = s_b[j] - centres[(size_t)p * d + j]; e += scales[(size_t)p * d + j] * df * df; }
      best = fmax(best, heights[p] * exp((-0.5 / d) * e));
    }
    const double v = bb_osz(10.0 - bb_block_max(best, s_red));
    f = v * v + pen;
  } else if (fid == 24) {
    const double* cond = aux;
    const double mu0 = 2.5, dd = 1.0, sfac = 1.0 - 0.5 / (sqrt(d + 20.0) - 4.1), mu1 = -sqrt((mu0 * mu0 - dd) / sfac);
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < d; i += BB_THREADS) {
      const double xh = 2.0 * (xopt[i] < 0.0 ? -s_x[i] : s_x[i]);
      s_a[i] = xh - mu0;
      s1 += (xh - mu0) * (xh - mu0);
      s2 += (xh - mu1) * (xh - mu1);
    }
    __syncthreads();
    bb_matvec(M, s_a, s_b, d);                                            // Q (xh - mu0)   (M slot holds Q)
    for (int i = tid; i < d; i += BB_THREADS) s_a[i] = cond[i] * s_b[i];
    __syncthreads();
    bb_matvec(R, s_a, s_b, d);                                            // z = R (cond .* ...)
    double c = 0.0;
    for (int i = tid; i < d; i += BB_THREADS) c += cos(two_pi * s_b[i]);
    const double S1 = bb_block_sum(s1, s_red), S2 = bb_block_sum(s2, s_red), C = bb_block_sum(c, s_red);
    f = fmin(S1, dd * d + sfac * S2) + 10.0 * (d - C) + 1e4 * pen;
  }
  if (tid == 0) { raw[slot] = f; oob[slot] = 0; }
}

// grid (B): one candidate per run, X[B][d]
__global__ __launch_bounds__(BB_THREADS) void k_bbob_eval(const double* __restrict__ tables, const int* __restrict__ fids,
                                                          BbobLayout L, const double* __restrict__ X, double lb, double ub,
                                                          double penalty, double* __restrict__ raw, int* __restrict__ oob) {
  bb_eval_one(tables, fids, L, X, blockIdx.x, blockIdx.x, blockIdx.x, lb, ub, penalty, raw, oob);
}

// grid (B, m): m candidates per run, X[B][m][d] -> raw[B][m], oob[B][m]; candidate j of run b as k_bbob_eval evaluates it alone
__global__ __launch_bounds__(BB_THREADS) void k_bbob_eval_many(const double* __restrict__ tables, const int* __restrict__ fids,
                                                               BbobLayout L, const double* __restrict__ X, int m, double lb, double ub,
                                                               double penalty, double* __restrict__ raw, int* __restrict__ oob) {
  const size_t slot = (size_t)blockIdx.x * m + blockIdx.y;
  bb_eval_one(tables, fids, L, X, blockIdx.x, slot, slot, lb, ub, penalty, raw, oob);
}

struct pcabo_objective {
  int device = 0, B = 0, d = 0;
  BbobLayout L;
  hipStream_t stream = nullptr;
  double *dTables = nullptr, *dX = nullptr, *dRaw = nullptr, *hX = nullptr, *hRaw = nullptr;
  int *dFid = nullptr, *dOob = nullptr, *hOob = nullptr;
  int cap_m = 1;                                     // candidates per run the staging buffers (dX, dRaw, dOob, hX, hRaw, hOob) hold
};

// The staging buffers for m candidates per run; they grow on the first call that needs them (the stream is idle between calls).
static bool bbob_reserve(pcabo_objective* o, int m) {
  if (m <= o->cap_m) return true;
  if (hipStreamSynchronize(o->stream) != hipSuccess) return false;
  void* dev[] = {o->dX, o->dRaw, o->dOob};
  for (void* p : dev) if (p) (void)hipFree(p);
  void* host[] = {o->hX, o->hRaw, o->hOob};
  for (void* p : host) if (p) (void)hipHostFree(p);
  o->dX = o->dRaw = o->hX = o->hRaw = nullptr;
  o->dOob = o->hOob = nullptr;
  o->cap_m = 0;
  const size_t slots = (size_t)o->B * m;
  const bool ok = hipMalloc((void**)&o->dX, slots * o->d * sizeof(double)) == hipSuccess &&
                  hipMalloc((void**)&o->dRaw, slots * sizeof(double)) == hipSuccess &&
                  hipMalloc((void**)&o->dOob, slots * sizeof(int)) == hipSuccess &&
                  hipHostMalloc((void**)&o->hX, slots * o->d * sizeof(double), hipHostMallocDefault) == hipSuccess &&
                  hipHostMalloc((void**)&o->hRaw, slots * sizeof(double), hipHostMallocDefault) == hipSuccess &&
                  hipHostMalloc((void**)&o->hOob, slots * sizeof(int), hipHostMallocDefault) == hipSuccess;
  if (ok) o->cap_m = m;
  return ok;
}

extern "C" {

int pcabo_bbob_table_doubles(int d) { return d >= 2 && d <= PCABO_MAXD ? bbob_layout(d).stride : PCABO_ERR_ARG; }

int pcabo_bbob_create(int device, int B, int d, const int* fid, const double* tables, pcabo_objective** out) {
  if (!out) return PCABO_ERR_ARG;
  *out = nullptr;
  if (B < 1 || d < 2 || d > PCABO_MAXD || !fid || !tables) return PCABO_ERR_ARG;
  for (int b = 0; b < B; ++b) if (fid[b] < 15 || fid[b] > 24) return PCABO_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return PCABO_ERR_HIP;
  pcabo_objective* o = new (std::nothrow) pcabo_objective();
  if (!o) return PCABO_ERR_HIP;
  o->device = device; o->B = B; o->d = d; o->L = bbob_layout(d);
  const size_t tb = (size_t)B * o->L.stride * sizeof(double);
  bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking) == hipSuccess &&
            hipMalloc((void**)&o->dTables, tb) == hipSuccess && hipMalloc((void**)&o->dX, (size_t)B * d * sizeof(double)) == hipSuccess &&
            hipMalloc((void**)&o->dRaw, B * sizeof(double)) == hipSuccess && hipMalloc((void**)&o->dFid, B * sizeof(int)) == hipSuccess &&
            hipMalloc((void**)&o->dOob, B * sizeof(int)) == hipSuccess &&
            hipHostMalloc((void**)&o->hX, (size_t)B * d * sizeof(double), hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&o->hRaw, B * sizeof(double), hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&o->hOob, B * sizeof(int), hipHostMallocDefault) == hipSuccess &&
            hipMemcpy(o->dTables, tables, tb, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(o->dFid, fid, B * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  *out = o;
  return ok ? PCABO_OK : PCABO_ERR_HIP;
}

int pcabo_bbob_destroy(pcabo_objective* o) {
  if (!o) return PCABO_ERR_ARG;
  (void)hipSetDevice(o->device);
  if (o->stream) { (void)hipStreamSynchronize(o->stream); (void)hipStreamDestroy(o->stream); }
  void* dev[] = {o->dTables, o->dX, o->dRaw, o->dFid, o->dOob};
  for (void* p : dev) if (p) (void)hipFree(p);
  void* host[] = {o->hX, o->hRaw, o->hOob};
  for (void* p : host) if (p) (void)hipHostFree(p);
  delete o;
  return PCABO_OK;
}

int pcabo_bbob_eval(pcabo_objective* o, const double* X, double lb, double ub, double penalty, double* raw, int* oob) {
  if (!o || !X || !raw) return PCABO_ERR_ARG;
  if (hipSetDevice(o->device) != hipSuccess || !bbob_reserve(o, 1)) return PCABO_ERR_HIP;
  const size_t xb = (size_t)o->B * o->d * sizeof(double);
  memcpy(o->hX, X, xb);
  if (hipMemcpyAsync(o->dX, o->hX, xb, hipMemcpyHostToDevice, o->stream) != hipSuccess) return PCABO_ERR_HIP;
  hipLaunchKernelGGL(k_bbob_eval, dim3(o->B), dim3(BB_THREADS), 0, o->stream, o->dTables, o->dFid, o->L, o->dX, lb, ub, penalty,
                     o->dRaw, o->dOob);
  if (hipMemcpyAsync(o->hRaw, o->dRaw, o->B * sizeof(double), hipMemcpyDeviceToHost, o->stream) != hipSuccess ||
      hipMemcpyAsync(o->hOob, o->dOob, o->B * sizeof(int), hipMemcpyDeviceToHost, o->stream) != hipSuccess ||
      hipStreamSynchronize(o->stream) != hipSuccess || hipGetLastError() != hipSuccess)
    return PCABO_ERR_HIP;
  memcpy(raw, o->hRaw, o->B * sizeof(double));
  if (oob) memcpy(oob, o->hOob, o->B * sizeof(int));
  return PCABO_OK;
}

int pcabo_bbob_eval_many(pcabo_objective* o, const double* X, int m, double lb, double ub, double penalty, double* raw, int* oob) {
  if (!o || !X || !raw || m < 1 || m > 65535) return PCABO_ERR_ARG;
  if (hipSetDevice(o->device) != hipSuccess || !bbob_reserve(o, m)) return PCABO_ERR_HIP;
  const size_t slots = (size_t)o->B * m, xb = slots * o->d * sizeof(double);
  memcpy(o->hX, X, xb);
  if (hipMemcpyAsync(o->dX, o->hX, xb, hipMemcpyHostToDevice, o->stream) != hipSuccess) return PCABO_ERR_HIP;
  hipLaunchKernelGGL(k_bbob_eval_many, dim3(o->B, m), dim3(BB_THREADS), 0, o->stream, o->dTables, o->dFid, o->L, o->dX, m, lb, ub,
                     penalty, o->dRaw, o->dOob);
  if (hipMemcpyAsync(o->hRaw, o->dRaw, slots * sizeof(double), hipMemcpyDeviceToHost, o->stream) != hipSuccess ||
      hipMemcpyAsync(o->hOob, o->dOob, slots * sizeof(int), hipMemcpyDeviceToHost, o->stream) != hipSuccess ||
      hipStreamSynchronize(o->stream) != hipSuccess || hipGetLastError() != hipSuccess)
    return PCABO_ERR_HIP;
  memcpy(raw, o->hRaw, slots * sizeof(double));
  if (oob) memcpy(oob, o->hOob, slots * sizeof(int));
  return PCABO_OK;
}

}  // extern "C"
