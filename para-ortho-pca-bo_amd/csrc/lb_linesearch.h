// More-Thuente line search of L-BFGS-B (dcsrch / dcstep of the published code), defined once for the host optimiser (lbfgsb.cpp:
// Lbfgsb::lnsrlb, built by g++) and the device-resident one (kernels_lbfgsb.hip: lb_lnsrlb, every lane the same scalars), which
// must take the same steps bit for bit.  Both translation units are compiled without contraction.
#pragma once
#include <math.h>            // fabs, fmax, fmin, sqrt on doubles, unqualified: the same spelling for g++ and hipcc
#if defined(__HIPCC__)
#define LB_LS_FN __host__ __device__ inline
#else
#define LB_LS_FN inline
#endif

struct LbLineSearch {
  int task = 0;              // 0 START, 1 FG, 2 CONVERGENCE, 3 WARNING, 4 ERROR
  int brackt = 0;
  int stage = 1;
  double ginit = 0, gtest = 0, gx = 0, gy = 0, finit = 0, fx = 0, fy = 0, stx = 0, sty = 0, stmin = 0, stmax = 0;
  double width = 0, width1 = 0;
};

LB_LS_FN void lb_dcstep(double* stx, double* fx, double* dx, double* sty, double* fy, double* dy, double* stp, double fp,
                        double dp, int* brackt, double stpmin, double stpmax) {
  const double sgnd = dp * (*dx / fabs(*dx));
  double stpf, stpc, stpq, theta, s, gamma, p, q, r;
  if (fp > *fx) {
    theta = 3.0 * (*fx - fp) / (*stp - *stx) + *dx + dp;
    s = fmax(fabs(theta), fmax(fabs(*dx), fabs(dp)));
    gamma = s * sqrt((theta / s) * (theta / s) - (*dx / s) * (dp / s));
    if (*stp < *stx) gamma = -gamma;
    p = (gamma - *dx) + theta;
    q = ((gamma - *dx) + gamma) + dp;
    r = p / q;
    stpc = *stx + r * (*stp - *stx);
    stpq = *stx + ((*dx / ((*fx - fp) / (*stp - *stx) + *dx)) / 2.0) * (*stp - *stx);
    if (fabs(stpc - *stx) < fabs(stpq - *stx)) stpf = stpc;
    else stpf = stpc + (stpq - stpc) / 2.0;
    *brackt = 1;
  } else if (sgnd < 0.0) {
    theta = 3.0 * (*fx - fp) / (*stp - *stx) + *dx + dp;
    s = fmax(fabs(theta), fmax(fabs(*dx), fabs(dp)));
    gamma = s * sqrt((theta / s) * (theta / s) - (*dx / s) * (dp / s));
    if (*stp > *stx) gamma = -gamma;
    p = (gamma - dp) + theta;
    q = ((gamma - dp) + gamma) + *dx;
    r = p / q;
    stpc = *stp + r * (*stx - *stp);
    stpq = *stp + (dp / (dp - *dx)) * (*stx - *stp);
    if (fabs(stpc - *stp) > fabs(stpq - *stp)) stpf = stpc;
    else stpf = stpq;
    *brackt = 1;
  } else if (fabs(dp) < fabs(*dx)) {
    theta = 3.0 * (*fx - fp) / (*stp - *stx) + *dx + dp;
    s = fmax(fabs(theta), fmax(fabs(*dx), fabs(dp)));
    gamma = s * sqrt(fmax(0.0, (theta / s) * (theta / s) - (*dx / s) * (dp / s)));
    if (*stp > *stx) gamma = -gamma;
    p = (gamma - dp) + theta;
    q = (gamma + (*dx - dp)) + gamma;
    r = p / q;
    if (r < 0.0 && gamma != 0.0) stpc = *stp + r * (*stx - *stp);
    else if (*stp > *stx) stpc = stpmax;
    else stpc = stpmin;
    stpq = *stp + (dp / (dp - *dx)) * (*stx - *stp);
    if (*brackt) {
      if (fabs(stpc - *stp) < fabs(stpq - *stp)) stpf = stpc;
      else stpf = stpq;
      if (*stp > *stx) stpf = fmin(*stp + 0.66 * (*sty - *stp), stpf);
      else stpf = fmax(*stp + 0.66 * (*sty - *stp), stpf);
    } else {
      if (fabs(stpc - *stp) > fabs(stpq - *stp)) stpf = stpc;
      else stpf = stpq;
      stpf = fmin(stpmax, stpf);
      stpf = fmax(stpmin, stpf);
    }
  } else {
    if (*brackt) {
      theta = 3.0 * (fp - *fy) / (*sty - *stp) + *dy + dp;
      s = fmax(fabs(theta), fmax(fabs(*dy), fabs(dp)));
      gamma = s * sqrt((theta / s) * (theta / s) - (*dy / s) * (dp / s));
      if (*stp > *sty) gamma = -gamma;
      p = (gamma - dp) + theta;
      q = ((gamma - dp) + gamma) + *dy;
      r = p / q;
      stpc = *stp + r * (*sty - *stp);
      stpf = stpc;
    } else if (*stp > *stx) stpf = stpmax;
    else stpf = stpmin;
  }
  if (fp > *fx) { *sty = *stp; *fy = fp; *dy = dp; }
  else {
    if (sgnd < 0.0) { *sty = *stx; *fy = *fx; *dy = *dx; }
    *stx = *stp; *fx = fp; *dx = dp;
  }
  *stp = stpf;
}

LB_LS_FN void lb_dcsrch(double f, double g, double* stp, double ftol, double gtol, double xtol, double stpmin, double stpmax,
                        LbLineSearch& s) {
  const double xtrapl = 1.1, xtrapu = 4.0, p5 = 0.5, p66 = 0.66;
  if (s.task == 0) {
    if (*stp < stpmin || *stp > stpmax || g >= 0.0) { s.task = 4; return; }
    s.brackt = 0; s.stage = 1; s.finit = f; s.ginit = g; s.gtest = ftol * s.ginit;
    s.width = stpmax - stpmin; s.width1 = s.width / p5;
    s.stx = 0.0; s.fx = s.finit; s.gx = s.ginit; s.sty = 0.0; s.fy = s.finit; s.gy = s.ginit;
    s.stmin = 0.0; s.stmax = *stp + xtrapu * *stp;
    s.task = 1;
    return;
  }
  const double ftest = s.finit + *stp * s.gtest;
  if (s.stage == 1 && f <= ftest && g >= 0.0) s.stage = 2;
  int task = 1;
  if (s.brackt && (*stp <= s.stmin || *stp >= s.stmax)) task = 3;
  if (s.brackt && s.stmax - s.stmin <= xtol * s.stmax) task = 3;
  if (*stp == stpmax && f <= ftest && g <= s.gtest) task = 3;
  if (*stp == stpmin && (f > ftest || g >= s.gtest)) task = 3;
  if (f <= ftest && fabs(g) <= gtol * (-s.ginit)) task = 2;
  if (task == 2 || task == 3) { s.task = task; return; }
  if (s.stage == 1 && f <= s.fx && f > ftest) {
    double fm = f - *stp * s.gtest, fxm = s.fx - s.stx * s.gtest, fym = s.fy - s.sty * s.gtest;
    double gm = g - s.gtest, gxm = s.gx - s.gtest, gym = s.gy - s.gtest;
    lb_dcstep(&s.stx, &fxm, &gxm, &s.sty, &fym, &gym, stp, fm, gm, &s.brackt, s.stmin, s.stmax);
    s.fx = fxm + s.stx * s.gtest; s.fy = fym + s.sty * s.gtest; s.gx = gxm + s.gtest; s.gy = gym + s.gtest;
  } else {
    lb_dcstep(&s.stx, &s.fx, &s.gx, &s.sty, &s.fy, &s.gy, stp, f, g, &s.brackt, s.stmin, s.stmax);
  }
  if (s.brackt) {
    if (fabs(s.sty - s.stx) >= p66 * s.width1) *stp = s.stx + p5 * (s.sty - s.stx);
    s.width1 = s.width;
    s.width = fabs(s.sty - s.stx);
  }
  if (s.brackt) { s.stmin = fmin(s.stx, s.sty); s.stmax = fmax(s.stx, s.sty); }
  else { s.stmin = *stp + xtrapl * (*stp - s.stx); s.stmax = *stp + xtrapu * (*stp - s.stx); }
  *stp = fmax(*stp, stpmin);
  *stp = fmin(*stp, stpmax);
  if ((s.brackt && (*stp <= s.stmin || *stp >= s.stmax)) || (s.brackt && s.stmax - s.stmin <= xtol * s.stmax))
    *stp = s.stx;
  s.task = 1;
}
