// Scalar maths of the acquisition, defined once for every kernel that evaluates it (kernels_acq.hip: k_acq_fused, k_acq_fast,
// k_acq_group, the GEMM scoring; kernels_lbfgsb.hip: lb_eval).  The paths promise each other's bits, so the operations and their
// order live here and nowhere else.  Each translation unit keeps its own contraction flag: what must be fused in all of them is
// spelled out with __fma_rn.
#pragma once

// Covariance of two points from their scaled squared distance sq = |xn - zn|^2 / l^2, and the radial factor of its gradient before
// the lengthscale: dks/dxn = rf / l^2 (xn - zn).  kernel 1: RBF, otherwise Matern 5/2.  The caller multiplies by 1 / l^2 in its own
// spelling (rf * inv_ls * inv_ls and rf * il2 round differently).
__device__ inline void acq_cov(double sq, int kernel, double* ks, double* rf) {
  const double s5 = 2.23606797749979;
  if (kernel == 1) {
    *ks = exp(-0.5 * sq);
    *rf = -*ks;
  } else {
    const double dist = sqrt(fmax(sq, 1e-30));
    const double e = exp(-s5 * dist);
    *ks = ((s5 * dist + 1.0) + (5.0 / 3.0) * (dist * dist)) * e;
    *rf = -(5.0 / 3.0) * (1.0 + s5 * dist) * e;
  }
}
// value only (the GEMM scoring): the unused factor is dead code after inlining, the compiler drops it
__device__ inline double acq_cov_value(double sq, int kernel) {
  double ks, rf;
  acq_cov(sq, kernel, &ks, &rf);
  return ks;
}

// ---- scalar log-EI helper, value and derivative (botorch/acquisition/analytic.py::_log_ei_helper)
__device__ inline void log_ei_helper(double u, double* h, double* dh) {
  const double inv_sqrt2 = 0.7071067811865476;
  const double inv_sqrt_2pi = 0.3989422804014327;
  const double log2pi = 1.8378770664093453;
  if (u > -1.0) {
    double phi = inv_sqrt_2pi * exp(-0.5 * u * u);
    double Phi = 0.5 * erfc(-inv_sqrt2 * u);
    double ei = phi + u * Phi;
    *h = log(ei);
    *dh = Phi / ei;
    return;
  }
  double log_phi = -0.5 * (u * u + log2pi);
  if (u > -1e6) {
    // botorch: w = log(erfcx(-u/sqrt2) |u|) + log(sqrt(pi/2)); h = log_phi + log1mexp(w).  With E = e^w formed
    // directly, log1mexp(w) = log1p(-E) and expm1(-w) = (1 - E)/E: the same conditioning (both routes lose
    // eps/(1 - E)), three transcendental calls fewer on the one wave every round waits for.
    const double ex = erfcx(-inv_sqrt2 * u);
    const double E = (ex * fabs(u)) * 1.2533141373155003;       // sqrt(pi/2)
    *h = log_phi + log1p(-E);
    const double dw = (u + 0.7978845608028654 / ex) + 1.0 / u;  // sqrt(2/pi)/erfcx + u + 1/u
    *dh = -u - dw * E / (1.0 - E);
  } else {
    *h = log_phi - 2.0 * log(fabs(u));
    *dh = -u - 2.0 / u;
  }
}

// Scalar chain of one query: mean, sigma, u -> value and the two coefficients of the gradient's chain rule (c_mu = d value / d mu_s,
// c_sg the factor of the |v|^2 part), from the summed |v|^2 (vv) and mu_s (mus).  acq: 0 log-EI, 1 PI, 2 UCB.
__device__ inline void acq_scalar_chain(double vv, double mus, double ym, double ysd, double best_f, int maximize, int acq,
                                        double* value, double* c_mu, double* c_sg) {
  const double mu = ym + ysd * mus;
  double var = (1.0 - vv) * (ysd * ysd);
  bool clamped = false;
  if (!(var >= 1e-10)) { var = 1e-10; clamped = true; }     // gpytorch min_variance (double)
  if (var < 1e-12) { var = 1e-12; clamped = true; }          // botorch _mean_and_sigma(min_var)
  const double sigma = sqrt(var);
  const double sgn = maximize ? 1.0 : -1.0;
  if (acq == 2) {
    // PCABO_ACQ_UCB: value = sgn mu + kappa sigma, kappa in the best_f slot - linear in mu and sigma, no u.
    // The one fused multiply-add is spelled out: left to the compiler, a b + c d is contracted one way in one kernel and the
    // other way in the next, and a run in a batch must take the bits it takes alone.
    const double kappa = best_f;
    *value = __fma_rn(kappa, sigma, sgn * mu);
    *c_mu = sgn * ysd;                                              // d value / d mu_s
    *c_sg = clamped ? 0.0 : kappa * (-(ysd * ysd) / sigma);         // dsigma = -s_y^2 g_sigma / sigma
    return;
  }
  double u = (mu - best_f) / sigma;
  u *= sgn;
  double val, dv_du, dv_dsig;
  if (acq == 0) {
    double h, dh;
    log_ei_helper(u, &h, &dh);
    val = h + log(sigma);
    dv_du = dh;
    dv_dsig = 1.0 / sigma;
  } else {
    val = 0.5 * erfc(-0.7071067811865476 * u);
    dv_du = 0.3989422804014327 * exp(-0.5 * u * u);
    dv_dsig = 0.0;
  }
  *value = val;
  // du = sgn dmu/sigma - u dsigma/sigma ; dsigma = -s_y^2 g_sigma / sigma (0 where the variance was clamped)
  *c_mu = dv_du * sgn * ysd / sigma;
  *c_sg = clamped ? 0.0 : (dv_dsig - dv_du * u / sigma) * (-(ysd * ysd) / sigma);
}
