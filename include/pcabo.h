/*
 * pcabo.h - C ABI of libpcabo.so: the MI355X (gfx950) implementation of the PCA_BO inner loop.
 *
 * The reference (IvanBanny/para-ortho-pca-bo) is pure Python and has no FFI; the four places
 * where its hot loop hands arithmetic to third-party CPU libraries are the boundary this
 * library replaces.  Each entry point below names the reference call
 * site (file:line under /root/reference) whose work it performs.
 *
 * Conventions
 *   - fp64 everywhere, row-major, caller owns every buffer passed in.
 *   - Pointers are HOST pointers unless the context is switched with pcabo_set_pointer_mode()
 *     to PCABO_PTR_DEVICE, in which case the bulk inputs/outputs (marked [bulk]) are device
 *     pointers on the context's device (e.g. torch tensor .data_ptr()); small scalar/vector
 *     results (marked [host]) are always written to host memory.
 *   - Every call returns 0 on success or a negative pcabo_status; nothing throws across the ABI.
 *     pcabo_last_error() returns a human-readable message for the last failure on a context.
 *   - A context owns one HIP stream plus all workspaces, sized at creation for (max_n, max_d,
 *     max_q).  A context is single-threaded; distinct contexts are independent (one per
 *     concurrent BO run; ctypes releases the GIL around calls).
 *   - There is NO CPU fallback: without a usable HIP device pcabo_ctx_create() fails with
 *     PCABO_ERR_HIP.
 */
#ifndef PCABO_H
#define PCABO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pcabo_ctx pcabo_ctx;

typedef enum {
  PCABO_OK = 0,
  PCABO_ERR_ARG = -1,      /* bad argument / size exceeds context capacity / call order */
  PCABO_ERR_NOT_PD = -2,   /* K + s2 I not positive definite after the jitter retries */
  PCABO_ERR_HIP = -3,      /* HIP runtime error (message in pcabo_last_error) */
  PCABO_ERR_NAN = -4,      /* NaN met in an acquisition gradient (botorch raises here) */
  PCABO_ERR_TIMEOUT = -5   /* device did not answer within the watchdog interval */
} pcabo_status;

enum { PCABO_KERNEL_MATERN52 = 0, PCABO_KERNEL_RBF = 1 };
/* PCABO_ACQ_UCB: botorch's UpperConfidenceBound, value = (maximize ? mean : -mean) + kappa * sigma with kappa = sqrt(beta).  It has
 * no best_f, so wherever an entry point takes `best_f` (`best_f[B]` in the pcabo_batch_* calls) that slot carries kappa instead:
 * finite and >= 0, else PCABO_ERR_ARG.  The caller takes the square root (botorch: of the float32 tensor torch.as_tensor(beta));
 * PCABO_OPT_BESTF_F32 applies to the slot as it does to best_f. */
enum { PCABO_ACQ_LOG_EI = 0, PCABO_ACQ_PI = 1, PCABO_ACQ_UCB = 2 };
enum { PCABO_PTR_HOST = 0, PCABO_PTR_DEVICE = 1 };

/* ABI version of this header (checked by the Python loader). */
int pcabo_abi_version(void);

/* Number of HIP devices visible (0 when none; never fails). */
int pcabo_device_count(void);

/* Create / destroy a per-run context on `device`.
 * max_n: largest number of evaluated points (budget); max_d: ambient dimension;
 * max_q: largest number of query points per pcabo_acq_eval call (>= raw_samples). */
int pcabo_ctx_create(int device, int max_n, int max_d, int max_q, pcabo_ctx** out);
int pcabo_ctx_destroy(pcabo_ctx* ctx);
int pcabo_set_pointer_mode(pcabo_ctx* ctx, int mode);
int pcabo_last_error(pcabo_ctx* ctx, char* buf, int buflen);

/* Per-context switches.
 * PCABO_OPT_RESIDENT (default 1): pcabo_optimize_acqf may serve all evaluations of a call from ONE resident launch of
 *   the acquisition kernel (query points through a mailbox); 0 = one launch per evaluation.  Same arithmetic, same bits.
 * PCABO_OPT_BESTF_F32 (default 1): best_f is rounded to float32 before use, as botorch does when the reference hands it
 *   a Python float (`torch.as_tensor(best_f)`, PCA_BO.py:199-203); 0 keeps all 64 bits (what botorch does when the
 *   objective returned a numpy float64 scalar).
 * PCABO_OPT_GROUP_ACQ (default 0; 1 for the contexts of a batch): value+gradient evaluations of up to 32 points run through the
 *   throughput kernel (one work-group per restart group of <= 5 points and 64-row slab) instead of the per-query
 *   latency kernels; implies one launch per evaluation.  Same formulas, another summation order (~1e-15 relative), so a
 *   run is bit-reproducible within a mode, not across modes.
 * PCABO_OPT_HIDDEN_TAIL (default 1; no effect on the contexts of a batch): work of an iteration that need not sit behind the
 *   factorisation is taken off the main stream's chain.  pcabo_gp_condition_end_eval copies the samples and forms their kernel
 *   vectors on a second stream of the context beside the Cholesky (they need only the Normalize bounds and ZnT; the sums with
 *   alpha follow behind it), and pcabo_inverse_map runs on the host from the pinned wPCA results (no launch, no wait).
 *   0 = one stream and the k_inverse_map launch.  Same operations in the same order per element: same bits. */
enum { PCABO_OPT_RESIDENT = 0, PCABO_OPT_BESTF_F32 = 1, PCABO_OPT_GROUP_ACQ = 2,
       PCABO_OPT_DEVICE_LBFGSB = 3 /* batches only, see pcabo_batch_set_option */,
       PCABO_OPT_HIDDEN_TAIL = 5 /* (4 was an option that has been removed: the number is not reused) */ };
int pcabo_set_option(pcabo_ctx* ctx, int option, int value);

/* Rows A-C (+D,J): rank-weighted PCA of the evaluated points.
 * Replaces PCA_BO._calculate_weights + _transform_points_to_reduced_space
 * (Algorithms/BayesianOptimization/PCA_BO.py:316-408), i.e. numpy + sklearn PCA().fit/transform.
 *   X[n*d]      [bulk] evaluated points
 *   f[n]        [bulk] objective values; used only when ranks == NULL (device ranking, ties
 *               broken by index)
 *   ranks[n]    [bulk] 1-based ranks (best = 1) as numpy's argsort(argsort(.))+1 gives them, or NULL
 *   noise[n*d]  [bulk] the N(0,1e-8) draw of PCA_BO.py:376 (numpy global RNG), or NULL for none
 *   n_components > 0 fixes k; otherwise k = #(cumsum(evr) <= var_threshold) + 1 clamped to [1, min(n,d)]
 * Outputs (any may be NULL):
 *   data_mean[d], pca_mean[d] [host]; comps[r*d] [host] all r=min(n,d) components (sklearn
 *   components_, rows sorted by decreasing variance, sign: max-|.| entry of each row positive);
 *   evr[r] [host]; *k [host]; Z[n*k] [bulk] reduced coordinates (PCA_BO.py:407).
 * The context keeps X-mean, the k leading components and Z on the device for the calls below. */
int pcabo_wpca(pcabo_ctx* ctx, const double* X, const double* f, const int64_t* ranks, int n, int d,
               int maximize, double var_threshold, int n_components, const double* noise,
               double* data_mean, double* pca_mean, double* comps, double* evr, int* k, double* Z);

/* Rows D-H: condition the exact GP on (Z, y).
 * Replaces PCA_BO._initialize_model (PCA_BO.py:502-545: SingleTaskGP(MaternKernel(2.5),
 * Standardize, Normalize)) and the lazy Gram/Cholesky/alpha/root-inverse that gpytorch performs
 * on the first posterior call inside optimize_acqf (PCA_BO.py:607).
 *   Z[n*k]           [bulk] reduced points, or NULL to use the Z of the last pcabo_wpca call
 *   y[n]             [bulk] objective values (un-standardised)
 *   norm_bounds[2*k] [host] Normalize bounds (lo row, hi row) or NULL for PCA_BO.py:514-518
 *   lengthscale, noise: model constants (reference values: ln 2 and exp(-5)); kernel: PCABO_KERNEL_*
 * On Cholesky breakdown jitter 1e-8, 1e-7, 1e-6 is added (psd_safe_cholesky) before PCABO_ERR_NOT_PD.
 * A K that is not finite - a column of Z in which all points agree and no norm_bounds: a Normalize range of 0 - ends
 * there too (gpytorch raises on the NaN); the context then holds no GP until the next successful conditioning. */
int pcabo_gp_condition(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k,
                       const double* norm_bounds, double lengthscale, double noise, int kernel);

/* The same in two halves: _begin stages the inputs and enqueues every kernel without waiting, _end waits,
 * checks the factorisation and performs the jitter retries.  Lets the host prepare the next phase (e.g. the
 * Sobol engine of the initial-condition draw) while the device conditions the GP. */
int pcabo_gp_condition_begin(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k,
                             const double* norm_bounds, double lengthscale, double noise, int kernel);
int pcabo_gp_condition_end(pcabo_ctx* ctx);

/* pcabo_gp_condition_end followed by pcabo_acq_eval(values only) with the evaluation enqueued behind the conditioning
 * instead of after the host has seen it finish (the 512 raw samples of botorch's gen_batch_initial_conditions,
 * PCA_BO.py:607-614, are drawn from the search box, which is known long before the factorisation ends).
 * Same results as the two calls. Xq[q*k] [bulk], val[q] [bulk] (device-pointer mode simply runs the two calls). */
int pcabo_gp_condition_end_eval(pcabo_ctx* ctx, const double* Xq, int q, double best_f, int maximize, int acq,
                                double* val);

/* Opt-in GP hyperparameter fit (not in the reference, which never trains its SingleTaskGP; DESIGN.md "GP hyperparameter fit").
 * theta = {noise s2, mean constant c, raw lengthscale rho}, lengthscale = softplus(rho); the model's initial values are
 * {exp(-5), 0, 0}.  loss = -[log N(y_s; c 1, K + s2 I) + log LogNormal(s2; -4, 1)] / n, what botorch's fit_gpytorch_mll minimises
 * for SingleTaskGP(MaternKernel(2.5), Standardize, Normalize).  Matern-5/2 only (PCABO_KERNEL_RBF: PCABO_ERR_ARG); exact
 * Cholesky with the jitter retries of pcabo_gp_condition at every n.  The other arguments as in pcabo_gp_condition.
 * Loss and gradient at theta; leaves the context conditioned at theta (acquisition calls may follow). */
int pcabo_gp_mll(pcabo_ctx* ctx, const double* Z /* NULL: Z of the last wPCA */, const double* y, int n, int k,
                 const double* norm_bounds, int kernel, const double* theta /*3*/, double* loss, double* grad /*3*/);
/* The whole fit from theta_inout: host L-BFGS-B with scipy's defaults (m 10, factr 1e7, pgtol 1e-5, maxls 20, maxiter = maxfun
 * = 15000, the published summation order), bound s2 >= 1e-4, one attempt.  On return theta_inout holds the fitted theta, *loss
 * its loss, and the context is conditioned there (acquisition calls follow directly).
 * info[4] = {iterations, evaluations, warnflag (scipy's: 0 converged, 1 limit, 2 abnormal), task (LBFGSB_* code of the
 * optimiser, or PCABO_FIT_TASK_NOT_PD when a trial theta could not be factored even with jitter, PCABO_FIT_TASK_DOMAIN when a
 * trial theta left the model's domain: a step so long that softplus(rho) underflows to 0, a non-finite value)}.  A fit that ends
 * abnormally keeps the last accepted iterate (or the start) and still returns PCABO_OK: the caller reads warnflag. */
#define PCABO_FIT_TASK_NOT_PD (-2)
#define PCABO_FIT_TASK_DOMAIN (-3)
int pcabo_gp_fit(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds, int kernel,
                 double* theta_inout /*3*/, double* loss, int* info /*4*/);
/* The same fit with one lengthscale per input (automatic relevance determination, MaternKernel(nu=2.5, ard_num_dims=k); DESIGN.md
 * "ARD lengthscales").  theta = {s2, c, rho_1 .. rho_k}, l_c = softplus(rho_c); the start is {exp(-5), 0, 0 .. 0}, and equal rho is
 * exactly the model of pcabo_gp_mll / pcabo_gp_fit.  Loss, prior, bound, optimiser, info, stops and error codes as there (Matern-5/2
 * only; a theta outside the domain - s2 <= 0, a lengthscale that is 0 or not finite - is PCABO_ERR_ARG, except that the fit, like
 * pcabo_gp_fit, clips a finite start s2 below its bound 1e-4 to the bound instead of refusing it).  grad[c + 2] =
 * d loss / d rho_c.  The fit alone adds the optimiser bound rho_c >= ln 2^-40 = -27.73 (a lengthscale of 2^-40 of the range, below
 * which a folded range is held anyway): it keeps the long trial steps that the flat directions of irrelevant inputs produce inside
 * the domain, and a start below it is clipped to it as one with s2 < 1e-4 is.  The context is left conditioned at theta and acquisition calls follow directly: the lengthscales are folded
 * into the Normalize ranges, (hi_c - lo_c) l_c, and the model runs at lengthscale 1 on them - the search box (pcabo_acq_bounds) is
 * not folded.  The next pcabo_gp_condition* / pcabo_wpca_gp_condition_begin returns to the unfolded model.
 * Single contexts only: on a member context of a batch both return PCABO_ERR_ARG (the lock-step batches fit one lengthscale). */
int pcabo_gp_mll_ard(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds, int kernel,
                     const double* theta /*2+k*/, double* loss, double* grad /*2+k or NULL*/);
int pcabo_gp_fit_ard(pcabo_ctx* ctx, const double* Z, const double* y, int n, int k, const double* norm_bounds, int kernel,
                     double* theta_inout /*2+k*/, double* loss, int* info /*4*/);

/* Rows A-H as ONE enqueue: pcabo_wpca immediately followed by pcabo_gp_condition_begin(Z = NULL,
 * norm_bounds = NULL), i.e. PCA_BO._transform_points_to_reduced_space + _initialize_model of one iteration
 * (PCA_BO.py:343-408 and :502-545) without the host round trip between them: the conditioning launches are queued
 * behind the projection before the host has seen k (the kernels read it on the device).  Arguments as in the two
 * calls (gp_noise = the likelihood noise, `noise` = the PCA_BO.py:376 draw).  Returns when the wPCA results are on the
 * host, with the conditioning still in flight: finish with pcabo_gp_condition_end().  With all five output pointers NULL
 * it returns right after the enqueue; pcabo_wpca_results() then waits for and delivers the wPCA results. */
int pcabo_wpca_gp_condition_begin(pcabo_ctx* ctx, const double* X, const double* f, const int64_t* ranks, int n,
                                  int d, int maximize, double var_threshold, int n_components, const double* noise,
                                  const double* y, double lengthscale, double gp_noise, int kernel,
                                  double* data_mean, double* pca_mean, double* comps, double* evr, int* k);

/* Second half of pcabo_wpca_gp_condition_begin when that was called with all five output pointers NULL (enqueue only):
 * waits for the wPCA results - the conditioning keeps running - and hands them out.  Between the two calls the host can
 * do work that only needs a guess of k (PCA_BO builds the scrambled Sobol engine of botorch's initial-condition draw with
 * the previous iteration's k while the eigen-decomposition runs, and rebuilds it in the rare case that k changed).
 * Must precede pcabo_acq_bounds / pcabo_gp_condition_end(_eval). */
int pcabo_wpca_results(pcabo_ctx* ctx, double* data_mean, double* pca_mean, double* comps, double* evr, int* k);

/* Row J: search box of the acquisition optimiser, PCA_BO.py:558-573. bounds[2*k] [host] (lo row, hi row).
 * May be called between pcabo_gp_condition_begin and _end: it then waits only for the statistics kernel, so the
 * raw samples of the initial-condition draw can be generated while the factorisation is still running. */
int pcabo_acq_bounds(pcabo_ctx* ctx, double* bounds);

/* Row I: batched acquisition value (+ gradient) at q query points of the reduced space.
 * Replaces LogExpectedImprovement / ProbabilityOfImprovement .forward + torch autograd as driven
 * by botorch (PCA_BO.py:199-203, 607-614).
 *   Xq[q*k] [bulk]; best_f as the reference passes it (current_best; it is rounded to float32
 *   like torch.as_tensor(python float) does; PCABO_ACQ_UCB: kappa, see the enum); val[q] [bulk]; grad[q*k] [bulk] or NULL. */
int pcabo_acq_eval(pcabo_ctx* ctx, const double* Xq, int q, double best_f, int maximize, int acq,
                   double* val, double* grad);
/* Name suggested by SURVEY.md 8b; identical to pcabo_acq_eval(..., PCABO_ACQ_LOG_EI, ...). */
int pcabo_logei(pcabo_ctx* ctx, const double* Xq, int q, double best_f, int maximize,
                double* val, double* grad);

/* What the conditioned GP predicts at q points of the reduced space: the reference's model.posterior(test_points)
 * (Algorithms/utils/visualization_utils.py:458-461).  Opt-in, not used by the BO loop (DESIGN.md "GP posterior queries").
 * Semantics: gpytorch's and botorch's for SingleTaskGP(MaternKernel | RBFKernel, Standardize, Normalize) without an output scale,
 * restated; parity with BoTorch itself is unpinned (the tests compare with this repository's own oracle).
 *   Xq[q*k] [bulk]; flags: 0 or PCABO_POST_OBS_NOISE; mean[q], var[q], cov[q*q] [bulk], each may be NULL (not all three).
 *   mean_a = y_mean + y_std sum_j alpha_j k(x_a, z_j).  After a fit y_mean carries the constant mean (m + s c); after an ARD fit the
 *            folded Normalize ranges and lengthscale 1 are used as they stand; in a batch after its fit every run reads its own model.
 *   var_a  = (1 - |v_a|^2) y_std^2, v = L^-1 k(Z, x_a): the latent variance, floored like gpytorch's (values below 1e-10, NaN
 *            included, become 1e-10).  With PCABO_POST_OBS_NOISE: ((1 - |v_a|^2) + s2) y_std^2, then the same floor; s2 is the
 *            likelihood noise the context was conditioned with (the fitted one after a fit).  Jitter the factorisation had to add
 *            is part of K, not of s2.  botorch's second floor (1e-12) belongs to its analytic acquisitions and is not applied.
 *   cov    = y_std^2 (k(Xq, Xq) [+ s2 I] - V^T V), full q x q, row-major, symmetric bit for bit, NOT floored (gpytorch's
 *            covariance_matrix is not); its diagonal is bit-equal to the variance of the same call before the floor.
 * PCABO_ERR_ARG, nothing launched: q < 1 or q > max_q; mean, var and cov all NULL; unknown flag bits; no GP in the context (never
 * conditioned, or the last conditioning ended PCABO_ERR_NOT_PD / not finite); between pcabo_gp_condition_begin and its _end.
 * The V (n x max_q) and cov (max_q^2) buffers are allocated by the first call that asks for a covariance and kept until destroy.
 * Returns when the results are there.  A call changes nothing the later calls of the context read: what follows is bit for bit
 * what it would have been without it. */
enum { PCABO_POST_OBS_NOISE = 1 };
int pcabo_gp_posterior(pcabo_ctx* ctx, const double* Xq, int q, int flags, double* mean, double* var, double* cov);

/* Joint samples of that posterior from the caller's base samples: MultivariateNormal.rsample(base_samples=...) behind botorch's
 * GPyTorchPosterior, restated; parity with BoTorch itself is unpinned (DESIGN.md "GP posterior samples").  Opt-in, not used by the BO
 * loop.  There is no device RNG: a draw is a function of (Xq, flags, base) alone.
 *   mean[q], cov[q*q]: exactly what pcabo_gp_posterior returns for the same Xq and flags (without PCABO_POST_CENTRED).
 *   A_j = cov + j y_std^2 I, j the first of 0, 1e-8, 1e-7, 1e-6 on which the Cholesky succeeds (the rungs of the GP's own
 *         factorisation, psd_safe_cholesky's for float64); Lc = chol(A_j), lower.
 *   samples[s*q + a] = mean_a + sum_{b <= a} Lc[a][b] base[s*q + b];  base[S*q], samples[S*q] [bulk], row-major.
 *   flags: PCABO_POST_OBS_NOISE as above; PCABO_POST_CENTRED: the mean is not added (the centred process; base = I_q then reads Lc).
 *   mean[q] [bulk] may be NULL; jitter_used [host] may be NULL: the rung j that was used.
 * PCABO_ERR_ARG, nothing launched: the refusals of pcabo_gp_posterior; base or samples NULL; S < 1 or S > PCABO_POST_MAX_SAMPLES;
 * unknown flag bits.  PCABO_ERR_NOT_PD: no rung could be factored; samples is not written.
 * The first sampling call of a context allocates one block (the padded factor, base and samples at their capacities, the
 * factorisation's own info word and scratch tiles) and, like a covariance query, the V / cov buffers; both are kept until destroy.
 * Like pcabo_gp_posterior a call changes nothing that later calls of the context read. */
enum { PCABO_POST_CENTRED = 2 };   /* pcabo_gp_posterior_sample only: pcabo_gp_posterior refuses it */
#define PCABO_POST_MAX_SAMPLES 1024
int pcabo_gp_posterior_sample(pcabo_ctx* ctx, const double* Xq, int q, int flags, const double* base, int S,
                              double* samples, double* mean /*q, may be NULL*/, double* jitter_used /*may be NULL*/);

/* Leave-one-out (LOO) predictions of the conditioned GP: for every observed point what the model says about it from the other
 * n - 1 points (Rasmussen & Williams 5.4.2).  Opt-in, not used by the BO loop (DESIGN.md "Leave-one-out predictions").
 * With R the root inverse, alpha the solved weights, ys the standardised targets (after a fit they carry the mean constant) and
 * (m', s) the Standardize statistics (y_mean_std of pcabo_get_gp_state), for i < n, n the context's own:
 *   d_i    = sum_{p >= i} R[p][i]^2     (K^-1)_ii, K as factored: the noise and any jitter rung included
 *   r_i    = alpha_i / d_i              standardised LOO residual
 *   mean_i = m' + s (ys_i - r_i)        prediction of y_i from the other n - 1 points, objective units
 *   var_i  = s^2 / d_i                  predictive variance of the OBSERVATION y_i (noise included); never floored: d_i >= R_ii^2 > 0
 *   z_i    = r_i sqrt(d_i)              standardised residual (y_i - mean_i) / sqrt(var_i); N(0, 1) for a calibrated model
 *   lpd_i  = -1/2 (log(2 pi) + log(var_i) + z_i^2)      log predictive density of y_i
 *   lpd_sum = sum_i lpd_i, added in index order on the host from the n values brought back: one comparable score per model.
 * The hyperparameters and the Standardize / Normalize statistics are those of the FULL data: this is the usual LOO identity, not a
 * refit of the transforms (nor of the hyperparameters) without point i.  The constant mean of a fit, folded ARD lengthscales and
 * jitter need no special case: they are inside R, alpha, ys and (m', s).
 *   mean[n], var[n], z[n], lpd[n], lpd_sum[1]: all [host] in either pointer mode; each may be NULL (not all five).
 * PCABO_ERR_ARG, nothing launched: all outputs NULL; no GP in the context (never conditioned, or the last conditioning ended
 * PCABO_ERR_NOT_PD / not finite); between pcabo_gp_condition_begin and its _end.
 * One launch, no workspace of its own.  Returns when the results are there.  Like pcabo_gp_posterior a call changes nothing that
 * later calls of the context read: what follows is bit for bit what it would have been without it. */
int pcabo_gp_loo(pcabo_ctx* ctx, double* mean /*n*/, double* var /*n*/, double* z /*n*/, double* lpd /*n*/, double* lpd_sum /*1*/);

/* Append p >= 1 points to the conditioned GP, one after the other (point i + 1 sees point i), and take them back: the model of
 * botorch's condition_on_observations / fantasize.  Opt-in, not used by the BO loop (DESIGN.md "Extending a conditioned GP").
 * Transforms and hyperparameters are HELD, only the data grow: the Normalize bounds, the Standardize statistics (m', s), the
 * lengthscale, the noise s2, a fit's mean constant and folded ARD ranges stay those of the last conditioning or fit; a new point may
 * lie outside the Normalize box.  With R = L^-1 as the library keeps it, per point x (k coordinates, reduced space) with value y:
 *   xn_c = (x_c - lo_c) / (hi_c - lo_c),  ks_j = k(xn, zn_j) for j < n,  v = R ks,  w = R^T v,
 *   d2 = (1 + s2 + rung) - |v|^2      rung: the jitter the conditioning's factorisation ended on (0 normally)
 *   L[n] = [v, sqrt(d2)],  R[n] = [-w, 1] / sqrt(d2),  ys_n = (y - m') / s,  n <- n + 1,  alpha = R^T (R ys) on the n + 1 points.
 *   PCABO_EXTEND_BELIEVER: yp may be NULL (it is not read) and ys_n = sum_j alpha_j ks_j, the model's own mean at the point.
 *   Zp[p*k] [bulk], yp[p] [bulk].  Every sum has one order: the same call on the same state gives the same bytes.
 * All or nothing: if d2 of a point is not positive and finite the call returns PCABO_ERR_NOT_PD with the context taken back to the n
 * it had on entry.  PCABO_ERR_ARG, nothing launched and nothing written: p < 1; n + p > max_n; Zp NULL; yp NULL without the believer
 * flag; a coordinate or value that is not finite (host-pointer mode); unknown flag bits; no conditioned GP; between
 * pcabo_gp_condition_begin and its _end; a member context of a batch (the lock-step form is pcabo_batch_gp_extend / pcabo_batch_gp_truncate;
 * pcabo_gp_extended on a member reads its batch's counts).
 * pcabo_gp_truncate takes back the points from n0 on, n_base <= n0 <= n (else PCABO_ERR_ARG), n_base the n of the last conditioning
 * or fit: the leading block of a triangular inverse is the inverse of the leading block, so this is bookkeeping plus alpha on n0
 * points.  After pcabo_gp_truncate(ctx, n_base) every later call returns the bytes it would have returned before the first extend.
 * pcabo_gp_extended reads both counts.  A new conditioning, fit or likelihood evaluation starts over: it sets n_base and forgets the
 * extension.  The search box (pcabo_acq_bounds) stays that of the conditioning throughout. */
enum { PCABO_EXTEND_BELIEVER = 1 };
int pcabo_gp_extend(pcabo_ctx* ctx, const double* Zp, const double* yp, int p, int flags);
int pcabo_gp_truncate(pcabo_ctx* ctx, int n0);
int pcabo_gp_extended(pcabo_ctx* ctx, int* n_base /*may be NULL*/, int* n /*may be NULL*/);

/* Rows M-N: multi-start L-BFGS-B over the acquisition (botorch gen_candidates_scipy semantics:
 * restarts are optimised jointly in groups of `batch_limit`, objective -sum_j acq(x_j), scipy
 * L-BFGS-B defaults m=10, factr=1e7 (ftol 2.22e-9), pgtol=1e-5, maxls=20, maxfun=15000).
 * Replaces botorch.optim.optimize_acqf's optimisation stage (PCA_BO.py:607-614).
 *   ics[num_restarts*k] [host] initial conditions; bounds[2*k] [host];
 *   cand[num_restarts*k] [host] clamped final points; vals[num_restarts] [host] acquisition there;
 *   info[4*ngroups] [host] or NULL: per group {iterations, function evaluations, warnflag, task};
 *   returns PCABO_OK; *failed (may be NULL) is set to 1 when a group ended abnormally (the case in
 *   which botorch re-draws initial conditions and retries once). */
int pcabo_optimize_acqf(pcabo_ctx* ctx, const double* ics, int num_restarts, int batch_limit,
                        const double* bounds, int maxiter, double best_f, int maximize, int acq,
                        double* cand, double* vals, int* info, int* failed);

/* Rows K-N of a single run in ONE call (host pointers only): score the n_raw raw samples - behind the conditioning when one is in
 * flight (pcabo_gp_condition_end_eval and its call-order rules), on the conditioned model otherwise (pcabo_acq_eval, values only)
 * -, pick num_restarts < n_raw of them as botorch's initialize_q_batch(eta) does on the generator whose state `blob` is
 * (pcabo_boltzmann_pick_rows for one row; the blob is ADVANCED in place), and run pcabo_optimize_acqf from them.  The variates of
 * the pick are drawn while the host would wait for the scores, and the optimiser's stepping helper is woken before that wait
 * (flags = PCABO_PROPOSE_NO_WAKE leaves it asleep until the optimiser needs it: the A/B switch of that one step).
 *   raw[n_raw*k], bounds[2*k] [host]; raw_vals[n_raw], ic_idx[num_restarts], ics[num_restarts*k] [host] out;
 *   cand, vals, info, failed as pcabo_optimize_acqf; phase_seconds[3] [host] or NULL: wait + score, pick, optimise (steady_clock).
 *   *picked = 1: everything was written.  *picked = 0: flag 1 of pcabo_boltzmann_pick_rows (no spread, or tied ratios) - raw_vals is written, the
 *   blob is byte for byte what it was, nothing was optimised: the caller takes botorch's other paths and calls pcabo_optimize_acqf.
 * PCABO_ACQ_PI, whose pick is botorch's non-negative variant, is refused.  Same bits as the separate calls. */
enum { PCABO_PROPOSE_NO_WAKE = 1 };
int pcabo_propose_acqf(pcabo_ctx* ctx, const double* raw, int n_raw, void* blob, double eta, int num_restarts, int batch_limit,
                       const double* bounds, int maxiter, double best_f, int maximize, int acq, int flags, double* raw_vals,
                       int64_t* ic_idx, double* ics, double* cand, double* vals, int* info, int* failed, int* picked,
                       double* phase_seconds);

/* Row O: x = z Ck + pca_mean + data_mean (PCA_BO.py:410-434). z[k] [host] -> x[d] [host]. */
int pcabo_inverse_map(pcabo_ctx* ctx, const double* z, double* x);

/* Introspection used by the parity tests (all [host] outputs, row-major n x n / vectors).
 * After pcabo_gp_mll_ard / pcabo_gp_fit_ard norm_bounds are the FOLDED Normalize bounds the model runs on:
 * hi_c = lo_c + (hi_c - lo_c) l_c (the model's lengthscale is then 1).
 * On a member context of a batch that is set aside (pcabo_batch_gp_extend) n is the number of points the run holds, not the batch's. */
int pcabo_get_gp_state(pcabo_ctx* ctx, double* K_chol /*n*n lower*/, double* Rinv /*n*n lower*/,
                       double* alpha /*n*/, double* y_mean_std /*2*/, double* norm_bounds /*2*k*/);
int pcabo_get_gram(pcabo_ctx* ctx, double* K /*n*n, symmetric, incl. noise*/);

/* Host-only L-BFGS-B (no device work): minimise a callback objective with box bounds, same
 * algorithm and defaults as scipy.optimize.minimize(method="L-BFGS-B").  Used by the CPU tests
 * to pin this library's optimiser against scipy itself.
 *   fg(x, g, user) returns f and fills g.  Returns warnflag (0 converged, 1 limit, 2 abnormal). */
typedef double (*pcabo_fg_callback)(const double* x, double* g, void* user);
int pcabo_lbfgsb_minimize(int nvar, double* x, const double* lower, const double* upper,
                          pcabo_fg_callback fg, void* user, int m, double factr, double pgtol,
                          int maxiter, int maxfun, int maxls, double* f_out, int* nit, int* nfev,
                          int* task_out);
/* The O(m n) loops of the host L-BFGS-B have AVX2 forms that take, bit for bit, the scalar loops' iterates (same operands,
 * same order, no fma); on by default where the CPU has AVX2.  0 selects the scalar loops (process-wide; the test that
 * compares the two uses it), 1 the default again.  Returns the previous setting. */
int pcabo_lbfgsb_set_vector_kernels(int enabled);
/* Summation order of the sums over the variables (d'd, g'd, r'r, W'd ...) in optimisers started by pcabo_lbfgsb_minimize from now
 * on: 0 (default) the published order - scipy's iterates; 1 the 64-lane tree order in which the device-resident optimiser
 * (PCABO_OPT_DEVICE_LBFGSB) steps: lane l adds terms l, l + 64, ..., then a balanced tree of adjacent pairs.  With 1 the host class
 * is the device's twin bit for bit (tests/test_gpu_device_lbfgsb.py); against scipy it is one more rounding of the same sums
 * (tests/test_lbfgsb_vs_scipy.py, tests/test_lbfgsb_divergence.py state what that does).  Returns the previous setting. */
int pcabo_lbfgsb_set_sum_order(int order);

/* Host-only helper for the initial-condition draw (botorch -> torch.quasirandom.SobolEngine, row K):
 * the matrix scramble of torch's `_sobol_engine_scramble_` on state[k*30] (in/out) with the k lower-
 * triangular 30x30 0/1 matrices ltm[k*30*30] (as drawn by torch.randint(...); entries on and above the diagonal are not
 * read - torch's .tril() need not be applied); bit-identical to torch, ~100x faster than torch's accessor loop.  The random
 * bits themselves still come from torch's generator. */
int pcabo_sobol_scramble(int64_t* state, const int64_t* ltm, int k);
/* The draw of such an engine (fresh: nothing generated yet), bit-identical to SobolEngine.draw(n, dtype=float64) followed by
 * botorch's map into the box, out[i*k + j] = lo[j] + rng[j] * u[i][j] (lo = rng = NULL: u itself).  state[k*30] after
 * pcabo_sobol_scramble, shift[k] = sum_b bit_b 2^b of the k x 30 shift bits (torch's `shift`). */
int pcabo_sobol_draw(const int64_t* state, const int64_t* shift, int k, int n, const double* lo, const double* rng, double* out);
/* The same for every run of a lock-step batch in one call: run r draws n points (n x ks[r]) into outs[r], mapped into the box
 * [lo(k), hi(k)] found at boxes + r * box_stride (the packing of pcabo_batch_acq_bounds); states[r] == NULL skips run r. */
int pcabo_sobol_draw_rows(const int64_t* const* states, const int64_t* const* shifts, const int* ks, int rows, int n,
                          const double* boxes, long long box_stride, double* const* outs);
/* torch's CPU generator restated for the host's pacing thread (csrc/host_entry.cpp): `blob` = the generator's state exactly as
 * torch.Generator.get_state() exports it (5056 bytes), read and ADVANCED in place - set_state(blob) afterwards leaves torch's
 * generator where torch's own call would have left it.  Every entry point that takes a blob refuses (PCABO_ERR_ARG) one that is not
 * seeded or whose `left` / `next` bookkeeping would read past the 624 state words.
 * pcabo_torch_randint2: torch.randint(2, (count,), generator=g) - the Sobol scramble bits of botorch's draw_sobol_samples.
 * pcabo_torch_multinomial_rows: torch.multinomial(weights[r], n_pick, replacement=False, generator=g_r) for `rows` rows, one
 *   generator each (blobs[r] == NULL: row skipped) - the Boltzmann pick of botorch's initialize_q_batch; out[rows][n_pick].
 * pcabo/hostrng.py verifies both against torch at import and keeps torch's own calls if they ever differ. */
int pcabo_torch_randint2(void* blob, int64_t count, int64_t* out);
int pcabo_torch_multinomial_rows(void* const* blobs, const double* weights, int rows, int n, int n_pick, int64_t* out);
/* botorch's initialize_q_batch (Boltzmann pick of the restarts' initial conditions) for `rows` runs in one call: vals[rows][n] raw-sample
 * scores, eta the temperature; out[rows][n_pick]; flags[rows]: 0 picked; 1 nothing picked here and the row's
 * generator is as it was - all values equal or a NaN among them, or the largest ratios of the draw tie (weights that overflowed or
 * underflowed; not at eta = 1): the caller runs torch's own initialize_q_batch on that generator; 2 skipped (blobs[r] == NULL). */
int pcabo_boltzmann_pick_rows(void* const* blobs, const double* vals, int rows, int n, int n_pick, double eta, int64_t* out, int* flags);

/* Device-time accounting: accumulated HIP-event time (ms, events recorded on the context's own
 * stream), launch count and ALGORITHMIC bytes / flops of the kernel groups since the last reset.
 * which: 0 wpca (5 kernels), 1 normalise+Gram (3 kernels), 2 Cholesky (2 kernels per 64-wide panel),
 * 3 root inverse + alpha (5 launches), 4 acquisition kernel, single-launch evaluations (<= 32 queries: the L-BFGS-B
 * rounds), 5 acquisition, large batches (two launches: partials + combine).
 * Enabled by pcabo_set_profiling(ctx, 1) (adds an event pair per bracketed group of launches; the reading of two events
 * recorded back to back, calibrated when profiling is switched on, is subtracted from every pair).
 * pcabo_get_profile_calibration: that reading (ms) and the reading of an event pair around an EMPTY kernel (ms), both medians
 * of 64, so that a caller can state raw event times next to the calibrated ones (bench.py does). */
int pcabo_set_profiling(pcabo_ctx* ctx, int enabled);
int pcabo_get_profile_calibration(pcabo_ctx* ctx, double* pair_ms, double* empty_kernel_ms);
int pcabo_get_profile(pcabo_ctx* ctx, int which, double* ms, int64_t* launches, double* bytes, double* flops);
int pcabo_reset_profile(pcabo_ctx* ctx);

/* ---- Batched contexts: B independent BO runs advancing in lock-step ---------------------------------------------------
 * The reference's outer loop is a list of independent runs (Algorithms/Experiment/ExperimentRunner.py:137-183: 30 instances
 * x functions x dimensions, one optimiser object each).  A batch holds B per-run contexts of equal capacity side by side in
 * one device slab and advances them together: every phase of rows A-H is ONE launch sequence with blockIdx.z = run (the
 * work-groups of all runs fill the chip together), the raw-sample scoring is one launch for all runs, and the L-BFGS-B
 * rounds of all runs are fed to shared acquisition launches (one per gang of runs and round; an active-query table names the
 * (run, query) pairs of the round).  The kernels and their per-run grids are those of the single context, so every run's
 * numbers are bit-identical to the same run in a context of its own.
 * All runs of a call share n and d (same budget / DoE sizes: the runs of one (function, dimension) cell or of several cells
 * with the same dimension); k and best_f are per run.  Per-run arrays are laid out [B][...] with the strides named below.
 * status[b] receives the pcabo_status of run b where a call can fail per run; the return value reports argument / HIP errors.
 * pcabo_batch_ctx(batch, b) is run b's context: the single-context calls above work on it (introspection, the rare retry of
 * one run), but not pcabo_ctx_destroy. */
typedef struct pcabo_batch pcabo_batch;
int pcabo_batch_create(int device, int B, int max_n, int max_d, int max_q, pcabo_batch** out);
int pcabo_batch_destroy(pcabo_batch* batch);
/* Worker threads of the L-BFGS-B phase (one gang of runs and one HIP stream each; default min(8, B)).
 * A worker spins while its launch is in flight: when several batches of one process advance side by side (one host thread
 * per batch - the reference's cells of different dimension, or two halves of one cell) give each its share of the cores.
 * Results do not depend on the number.  Not during a call on this batch. */
int pcabo_batch_set_workers(pcabo_batch* batch, int workers);
/* PCABO_OPT_GROUP_ACQ (default 1): the L-BFGS-B rounds of the batch go through the throughput kernel (k_acq_group); 0: through
 * the per-query kernels a stand-alone context uses by default - a run of the batch is then bit-identical to the same run in a
 * context of its own with default options (with 1 it is bit-identical to such a context with PCABO_OPT_GROUP_ACQ set).
 * PCABO_OPT_DEVICE_LBFGSB (default 0): 1 = pcabo_batch_optimize_acqf runs every restart group's whole L-BFGS-B optimisation
 *   (gen_candidates_scipy of PCA_BO.py:607-614) inside ONE kernel launch, a work-group per group: evaluate, step, next point
 *   without a host round trip (csrc/kernels_lbfgsb.hip; needs n <= 512, k <= 40, batch_limit <= 5 and finite bounds - other
 *   calls take the host-paced path).  Its evaluation sums in an order of its own (a third arithmetic mode, ~1e-15 relative from
 *   the other two).  2 = the same evaluation kernel driven by the HOST's L-BFGS-B, one launch per round: slow, the reference
 *   the device stepping is compared with bit for bit (tests/test_gpu_device_lbfgsb.py). */
int pcabo_batch_set_option(pcabo_batch* batch, int option, int value);
/* Shapes the device-resident optimiser (PCABO_OPT_DEVICE_LBFGSB = 1) covers: points n <= *max_n, reduced dimension k <= *max_k,
 * batch_limit <= *max_group.  A call beyond them is NOT served by it: pcabo_batch_optimize_acqf takes the host-paced path for that
 * call (pcabo_batch_optimize_acqf_begin returns 1), i.e. ANOTHER arithmetic mode.  A driver that promises one trajectory per seed
 * therefore decides per RUN, before it starts, from (budget, dimension) - pcabo/batchrun.py refuses acq_kernel="device" for a
 * run that could leave these limits, Algorithms/Experiment/ExperimentRunner.py resolves the mode per dimension of the experiment.
 * Host code; no device needed. */
int pcabo_device_lbfgsb_limits(int* max_n, int* max_k, int* max_group);
int pcabo_batch_last_error(pcabo_batch* batch, char* buf, int buflen);
pcabo_ctx* pcabo_batch_ctx(pcabo_batch* batch, int b);

/* Rows A-H of all runs as one enqueue (pcabo_wpca_gp_condition_begin for B runs).  X[B][n*d], ranks[B][n], noise[B][n*d] or
 * NULL, y[B][n].  Returns after the enqueue; pcabo_batch_wpca_results waits for the wPCA part only. */
/* Doubles between the blocks of two runs in the X / noise / y arrays handed to pcabo_batch_wpca_gp_condition_begin (0 = dense,
 * the default: n*d, n*d, n).  A driver that keeps X as [B][budget][d] passes budget*d and saves a dense copy per iteration. */
int pcabo_batch_set_input_strides(pcabo_batch* batch, size_t x_stride, size_t noise_stride, size_t y_stride);
int pcabo_batch_wpca_gp_condition_begin(pcabo_batch* batch, const double* X, const int64_t* ranks, const double* noise,
                                        const double* y, int n, int d, int maximize, double var_threshold,
                                        int n_components, double lengthscale, double gp_noise, int kernel);
/* Rows D-H of all runs without the weighted PCA (pcabo_gp_condition_begin for B runs): the reference's Vanilla_BO conditions its
 * GP on the raw d-dimensional points with Normalize switched off (Vanilla_BO.py:166-196) - the caller passes identity bounds.
 * Z[B][n*k], y[B][n] (strides: pcabo_batch_set_input_strides), norm_bounds[2*k] (lo[k], hi[k], the same for every run) or NULL
 * (bounds from the data, as for PCA_BO).  Continue with pcabo_batch_gp_condition_end_eval / pcabo_batch_optimize_acqf. */
int pcabo_batch_gp_condition_begin(pcabo_batch* batch, const double* Z, const double* y, int n, int k, const double* norm_bounds,
                                   double lengthscale, double gp_noise, int kernel);
/* data_mean[B][d], pca_mean[B][d], comps[B][d*d] (the first min(n,d)*d entries of each block), evr[B][d], k[B]; any may be NULL */
int pcabo_batch_wpca_results(pcabo_batch* batch, double* data_mean, double* pca_mean, double* comps, double* evr, int* k);
/* Row J for every run: bounds[B][2*max_d], run b's block holds lo[k_b] then hi[k_b]. */
int pcabo_batch_acq_bounds(pcabo_batch* batch, double* bounds);
/* Wait for the conditioning of all runs and score q points per run (values only; the raw samples of
 * gen_batch_initial_conditions), enqueued behind the conditioning.  Xq[B][q*max_d]: run b's block holds a dense q x k_b array;
 * best_f[B]; val[B][q]; status[B] (PCABO_ERR_NOT_PD for a run whose factorisation failed after the jitter retries). */
int pcabo_batch_gp_condition_end_eval(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize,
                                      int acq, double* val, int* status);
/* Score q points per run on the batch's model AS IT STANDS - fitted or not, extended by pcabo_batch_gp_extend or not: values only,
 * the launches of pcabo_batch_gp_condition_end_eval (the GEMM scoring from q = 64, the per-query kernels below), every run's values
 * bit for bit those of pcabo_acq_eval(values only) on the same run in a context of its own with the same extension.  What the later
 * proposals of an iteration are scored with: pcabo_batch_gp_condition_end_eval ENDS a conditioning and refuses
 * an unfitted batch once that has happened.  Arrays as there.  Nothing of the model's phase changes and no run is redone alone.
 * status[B] (may be NULL): PCABO_ERR_ARG for a run parked by pcabo_batch_set_active, set aside, or without a GP - skipped, its block
 * of val left alone.  PCABO_ERR_ARG, nothing launched: a bad argument; no conditioned batch; a conditioning that has not been waited
 * for; a _begin half of the batch (this call's included) not yet ended.  _begin enqueues and returns, _end waits and collects. */
int pcabo_batch_acq_score(pcabo_batch* batch, const double* Xq /*[B][q*max_d]*/, int q, const double* best_f /*[B]*/, int maximize,
                          int acq, double* val /*[B][q]*/, int* status /*[B]*/);
int pcabo_batch_acq_score_begin(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq);
int pcabo_batch_acq_score_end(pcabo_batch* batch, int q, double* val, int* status);
/* pcabo_gp_posterior for every run in one launch sequence, each run bit for bit what it takes alone.  Host pointers.
 * Xq[B][q*max_d]: run b's block holds a dense q x k_b array; mean[B][q], var[B][q], cov[B][q*q], each may be NULL (not all three).
 * status[B] (may be NULL): PCABO_ERR_ARG for a run parked by pcabo_batch_set_active and for a run whose factorisation failed - both
 * are skipped, their output blocks left as they are.  Needs a batch whose conditioning has been waited for
 * (pcabo_batch_gp_condition_end_eval*, pcabo_batch_gp_fit): PCABO_ERR_ARG otherwise and for the refusals of pcabo_gp_posterior.
 * The runs' V and cov buffers are ONE allocation made by the first call that asks for a covariance. */
int pcabo_batch_gp_posterior(pcabo_batch* batch, const double* Xq, int q, int flags, double* mean, double* var, double* cov,
                             int* status);
/* pcabo_gp_posterior_sample for every run in one launch sequence, each run bit for bit what it takes alone.  Host pointers.
 * Xq[B][q*max_d] as above; base[B][S*q], samples[B][S*q]; mean[B][q], jitter_used[B], status[B] may be NULL.
 * status[b]: PCABO_ERR_ARG for a parked run and for a run without a GP (skipped, their output blocks left as they are);
 * PCABO_ERR_NOT_PD for a run none of whose rungs could be factored (its samples are not written) - the rungs after the first are
 * tried for such a run alone and the other runs are not held up.  The refusals of pcabo_batch_gp_posterior and of
 * pcabo_gp_posterior_sample apply.  The runs' sample blocks are ONE allocation made by the first call. */
int pcabo_batch_gp_posterior_sample(pcabo_batch* batch, const double* Xq /*[B][q*max_d]*/, int q, int flags,
                                    const double* base /*[B][S*q]*/, int S, double* samples /*[B][S*q]*/,
                                    double* mean /*[B][q]*/, double* jitter_used /*[B]*/, int* status /*[B]*/);
/* pcabo_gp_loo for every run in ONE launch and one strided copy back, each run bit for bit what it takes alone.  Host pointers.
 * mean[B][n], var[B][n], z[B][n], lpd[B][n], lpd_sum[B], each may be NULL (not all five); n is the batch's.  After
 * pcabo_batch_gp_fit / _ard every run reads its own model.  status[B] (may be NULL): PCABO_ERR_ARG for a run parked by
 * pcabo_batch_set_active and for a run without a GP - both are skipped, their output blocks left as they are.  PCABO_ERR_ARG with
 * nothing launched: the refusals of pcabo_gp_loo; a conditioning that has not been waited for or a _begin call without its _end. */
int pcabo_batch_gp_loo(pcabo_batch* batch, double* mean /*[B][n]*/, double* var, double* z, double* lpd, double* lpd_sum /*[B]*/,
                       int* status /*[B]*/);
/* pcabo_gp_extend / pcabo_gp_truncate / pcabo_gp_extended for the runs of a batch in lock-step: ONE launch sequence per point for all
 * runs, one wait per call.  Host pointers.  Zp[B][p*max_d]: run b's block holds a dense p x k_b array (packed like Xq of
 * pcabo_batch_gp_posterior); yp[B][p], or NULL with PCABO_EXTEND_BELIEVER (it is then not read); flags: 0 or PCABO_EXTEND_BELIEVER.
 * Per run the semantics are exactly those of pcabo_gp_extend: transforms and hyperparameters held (after pcabo_batch_gp_fit / _ard
 * every run's own noise, 1 / lengthscale, mean constant and folded ARD ranges), the points appended one after the other, the rung of
 * the run's own factorisation.  Every run that takes part ends with the bytes (L, R, alpha, y_s, ZnT, AT, nrm) it would have in a
 * context of its own, conditioned or fitted on the same data and extended with the same points.  All runs share n: on success the
 * batch's n becomes n + p and n_base is held; a new conditioning, fit or likelihood evaluation of the batch starts over from n_base.
 * Runs that take no part - parked by pcabo_batch_set_active, without a GP, or set aside (below): status[b] = PCABO_ERR_ARG; their
 * blocks of Zp / yp are not read and none of their model bytes is written, by the extend or by the truncate that follows.
 * A pivot that fails in run b (d2 not positive and finite): run b ALONE is taken back to the bytes it had on entry, status[b] =
 * PCABO_ERR_NOT_PD; the other runs keep their p points and the call returns PCABO_OK, the failure in status and in
 * pcabo_batch_last_error.
 * SET ASIDE: a run with a GP that did not go along with an extend (its pivot failed, or it was parked) holds fewer points than its
 * batch; it is out of step and is skipped like a run without a GP by every batched model call (posterior, sample, loo, optimise,
 * device_acq_eval, extend) and by the single-context calls on pcabo_batch_ctx(b), until a pcabo_batch_gp_truncate with n0 <= the n
 * of entry of the extend it missed - in particular n_base.  From then on it is live again with the bytes it had at n0.  A new
 * conditioning or fit clears the mark as well; a scoring of the extended batch (pcabo_batch_gp_condition_end_eval* after a fit)
 * does not: it skips the run (status[b] = PCABO_ERR_ARG, its block of val left alone).  The one call that still answers for such a
 * run is the reader pcabo_get_gp_state on pcabo_batch_ctx(b), which launches nothing: it hands out the factors at the n the run holds.  While n > n_base pcabo_batch_set_active refuses to change a flag (PCABO_ERR_ARG).
 * PCABO_ERR_ARG, nothing launched and nothing written: p < 1; n + p > max_n; Zp NULL; yp NULL without the believer flag; unknown
 * flag bits; a coordinate or value of a run that takes part that is not finite; no conditioned batch; a conditioning or a _begin
 * half of the batch not yet ended; truncate with n0 outside n_base .. n.
 * pcabo_batch_gp_truncate takes the points from n0 on back for the runs that hold rows beyond n0 (n0 == n: nothing to do); after a
 * truncate to n_base every later call of every run returns the bytes it would have returned before the first extend.
 * status[B] may be NULL.  pcabo_batch_gp_extended reads the batch's counts; either pointer may be NULL. */
int pcabo_batch_gp_extend(pcabo_batch* batch, const double* Zp /*[B][p*max_d]*/, const double* yp /*[B][p] or NULL*/, int p, int flags,
                          int* status /*[B], may be NULL*/);
int pcabo_batch_gp_truncate(pcabo_batch* batch, int n0, int* status /*[B], may be NULL*/);
int pcabo_batch_gp_extended(pcabo_batch* batch, int* n_base, int* n);
/* Rows M-N for every run (pcabo_optimize_acqf semantics per run).  ics[B][num_restarts*max_d] (dense num_restarts x k_b per
 * block), bounds[B][2*max_d] as pcabo_batch_acq_bounds gives them, best_f[B]; cand[B][num_restarts*max_d] (dense per block),
 * vals[B][num_restarts], info[B][4*ngroups] or NULL, failed[B], status[B].
 * Runs that are not optimised, in every mode of PCABO_OPT_DEVICE_LBFGSB and for the _begin / _end halves alike: a run parked by
 * pcabo_batch_set_active gets status[b] = PCABO_ERR_ARG, a run WITHOUT A GP - its conditioning ended on PCABO_ERR_NOT_PD, or it is set
 * aside by pcabo_batch_gp_extend - gets status[b] = PCABO_ERR_NOT_PD; failed[b] = 0 for both, their blocks of ics and bounds are not
 * read and their blocks of cand, vals and info are left as they are.  The call itself returns PCABO_OK. */
int pcabo_batch_optimize_acqf(pcabo_batch* batch, const double* ics, int num_restarts, int batch_limit,
                              const double* bounds, int maxiter, const double* best_f, int maximize, int acq,
                              double* cand, double* vals, int* info, int* failed, int* status);
/* The two waiting calls of an iteration in halves, for a caller that advances SEVERAL batches from one thread (the reference's
 * outer loop over runs, ExperimentRunner.py:137-183, interleaved instead of threaded): _begin enqueues and returns, _end waits
 * and collects, pcabo_batch_busy tells whether the batch's stream still has work (1) or a waiting call would return at once (0).
 * pcabo_batch_optimize_acqf_begin needs PCABO_OPT_DEVICE_LBFGSB = 1 (the whole optimisation is one launch); it returns 1 -
 * nothing enqueued - when the call does not qualify for it, and the caller then uses pcabo_batch_optimize_acqf.  The arrays
 * handed to a _begin are read before it returns. */
int pcabo_batch_busy(pcabo_batch* batch);
int pcabo_batch_gp_condition_end_eval_begin(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq);
int pcabo_batch_gp_condition_end_eval_end(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize,
                                          int acq, double* val, int* status);
int pcabo_batch_optimize_acqf_begin(pcabo_batch* batch, const double* ics, int num_restarts, int batch_limit,
                                    const double* bounds, int maxiter, const double* best_f, int maximize, int acq);
int pcabo_batch_optimize_acqf_end(pcabo_batch* batch, int num_restarts, int batch_limit, double* cand, double* vals, int* info,
                                  int* failed, int* status);
int pcabo_batch_inverse_map_begin(pcabo_batch* batch, const double* z);
int pcabo_batch_inverse_map_end(pcabo_batch* batch, double* x);
/* Park / unpark runs: active[B]; a parked run still goes through the lock-step launches of rows A-K but is skipped by
 * pcabo_batch_optimize_acqf (status PCABO_ERR_ARG).  For runs that failed the way the reference's would (botorch raises on a
 * NaN acquisition gradient, reached once the reference's unclipped out-of-box candidates have blown up the search box).
 * PCABO_ERR_ARG for a call that would change a flag while points appended by pcabo_batch_gp_extend have not been taken back. */
int pcabo_batch_set_active(pcabo_batch* batch, const int* active);
/* Device time of the phases of the last pcabo_batch_wpca_gp_condition_begin (HIP events on the batch's stream; call once
 * that conditioning has been waited for): ms[0] rows A-C, ms[1] Normalize + Gram, ms[2] Cholesky, ms[3] root inverse + alpha. */
int pcabo_batch_set_profiling(pcabo_batch* batch, int enabled);
int pcabo_batch_get_profile(pcabo_batch* batch, double* ms);
/* Row O for every run: z[B][max_d] (k_b entries used) -> x[B][d]. */
int pcabo_batch_inverse_map(pcabo_batch* batch, const double* z, double* x);
/* Value and gradient of the acquisition (botorch LogExpectedImprovement / ProbabilityOfImprovement + autograd, PCA_BO.py:199-203,
 * 681-682) at q <= 32 points per run through the evaluation of the device-resident optimiser (PCABO_OPT_DEVICE_LBFGSB on;
 * n <= 512, k <= 40).  Xq[B][q*max_d]: run b's points packed with stride k_b; val[B][q]; grad[B][q*max_d], same packing.
 * For diagnostics and parity tests: pcabo_batch_optimize_acqf evaluates inside its own launch. */
int pcabo_batch_device_acq_eval(pcabo_batch* batch, const double* Xq, int q, const double* best_f, int maximize, int acq,
                                double* val, double* grad);
/* The opt-in GP hyperparameter fit (pcabo_gp_mll / pcabo_gp_fit) for the B runs of a batch in lock-step.  Both work on the inputs
 * of the last pcabo_batch_wpca_gp_condition_begin / pcabo_batch_gp_condition_begin (their Z, y and Normalize bounds are still on
 * the device; the lengthscale and noise given there are the model of the runs that do not take part).  Every run has its own
 * theta = {s2, c, rho}; one round is ONE launch sequence for all runs (conditioning + likelihood kernels, one wait), and every
 * run takes bit for bit the evaluations - and so the fit - it takes alone through pcabo_gp_mll / pcabo_gp_fit on the same Z, y.
 * theta[B][3], loss[B], grad[B][3] (or NULL), info[B][4] and the status codes as in pcabo_gp_fit; status[B]: PCABO_OK,
 * PCABO_ERR_ARG for a run parked by pcabo_batch_set_active (it is skipped) or a theta outside the model's domain,
 * PCABO_ERR_NOT_PD for a run that could not be factored even with the jitter retries (done for that run alone; a trial theta of
 * a fit that fails so ends that run's fit with warnflag 2 at its last accepted iterate, the other runs go on).  Matern-5/2 only.
 * On return every run's context is conditioned at its own theta (for pcabo_batch_gp_fit: its result; a run that has finished
 * rests there while the others step), the batched acquisition launches and the single-context calls on pcabo_batch_ctx(b) use
 * that model, and pcabo_batch_gp_condition_end_eval* scores it (the wait it would have done is over already).  The next
 * conditioning call returns the batch to the shared model.  pcabo_batch_gp_fit_rounds: launch sequences of the last call. */
int pcabo_batch_gp_mll(pcabo_batch* batch, const double* theta /*B*3*/, double* loss /*B*/, double* grad /*B*3*/, int* status /*B*/);
int pcabo_batch_gp_fit(pcabo_batch* batch, double* theta_inout /*B*3*/, double* loss /*B*/, int* info /*B*4*/, int* status /*B*/);
int pcabo_batch_gp_fit_rounds(pcabo_batch* batch);
/* The same two calls with one lengthscale per input (pcabo_gp_mll_ard / pcabo_gp_fit_ard for the B runs in lock-step).  Row b of
 * theta (and of grad) starts ld_theta doubles behind row b - 1 and holds {s2, c, rho_1 .. rho_{k_b}}, k_b the run's own reduced
 * dimension; ld_theta >= 2 + max_b k_b.  What lies beyond 2 + k_b in a row is ignored on input and left alone on output.
 * Every run takes bit for bit the evaluations and the fit it takes alone through pcabo_gp_mll_ard / pcabo_gp_fit_ard; a run that
 * takes part is left conditioned with its lengthscales folded into its Normalize ranges (pcabo_debug_gp_state), a parked run at
 * the unfolded shared model.  Status codes, refusals and what follows the call as above; PCABO_ERR_ARG also for a ld_theta that
 * is too small.  All runs of one call have this form of the model: the shared-lengthscale calls above are the other form. */
int pcabo_batch_gp_mll_ard(pcabo_batch* batch, const double* theta /*B*ld_theta*/, int ld_theta, double* loss /*B*/,
                           double* grad /*B*ld_theta*/, int* status /*B*/);
int pcabo_batch_gp_fit_ard(pcabo_batch* batch, double* theta_inout /*B*ld_theta*/, int ld_theta, double* loss /*B*/,
                           int* info /*B*4*/, int* status /*B*/);

/* ---- BBOB f15-f24 objectives on the device, for runs that advance in lock-step ---------------------------------------
 * The reference evaluates `problem(x)` on the host, one candidate per BO iteration (PCA_BO.py:263; the problems come from
 * ioh, ExperimentRunner.py:90).  With B runs in lock-step their B candidates are evaluated in one launch.
 * tables[B][pcabo_bbob_table_doubles(d)]: per run [x_opt(d) | R(d*d) | M(d*d) | aux], generated on the host by the seeded
 * legacy generators (pcabo/bbob.py builds them; layout in pcabo/bbob_device.py).  fid[B] in 15..24.
 * pcabo_bbob_eval: X[B][d] candidates -> raw[B] (value WITHOUT f_opt; `penalty` for a candidate outside [lb, ub]^d, which is
 * not evaluated: PCA_BO.py:248-263) and oob[B] (may be NULL).
 * pcabo_bbob_eval_many: m >= 1 candidates per run in ONE launch (grid B x m), X[B][m][d] -> raw[B][m], oob[B][m] (may be NULL):
 * candidate j of run b gets the bytes pcabo_bbob_eval gives it alone (the same work-group code, one work-group per candidate).
 * For the q candidates a run proposes per iteration.  The staging buffers grow on the first call that needs
 * them.  PCABO_ERR_ARG: m < 1 (or > 65535, the grid's second dimension), a NULL obj, X or raw. */
typedef struct pcabo_objective pcabo_objective;
int pcabo_bbob_table_doubles(int d);
int pcabo_bbob_create(int device, int B, int d, const int* fid, const double* tables, pcabo_objective** out);
int pcabo_bbob_destroy(pcabo_objective* obj);
int pcabo_bbob_eval(pcabo_objective* obj, const double* X, double lb, double ub, double penalty, double* raw, int* oob);
int pcabo_bbob_eval_many(pcabo_objective* obj, const double* X, int m, double lb, double ub, double penalty, double* raw, int* oob);

/* ---- Final gather of best-so-far values across the GPUs of a node -------------------------------------
 * Runs are independent (ExperimentRunner.py:137-183: one optimiser object per (function, dimension, instance)), so the
 * multi-GPU path has NO collective inside the loop; the one exchange of the design is an all-gather of each rank's
 * best-so-far values after its runs, over RCCL (xGMI inside a node).  One process per GPU:
 *   rank 0:      pcabo_comm_unique_id(id)            128 bytes (ncclUniqueId); the CALLER hands them to the other ranks
 *                                                    (a file, the launcher's environment, its own store)
 *   every rank:  pcabo_comm_create(id, world, rank, device, &comm)       (collective: returns once all ranks have joined)
 *                pcabo_gather_best(comm, local, n_local, all)            all[world * n_local] [host], rank-major; n_local equal on all ranks
 *                pcabo_comm_destroy(comm)
 * librccl.so is opened on first use (no link-time dependency).  pcabo/distributed.py offers the same gather through
 * torch.distributed for callers that already run under it (bench.py does). */
typedef struct pcabo_comm pcabo_comm;
int pcabo_comm_unique_id(char* id128);
int pcabo_comm_create(const char* id128, int world, int rank, int device, pcabo_comm** out);
int pcabo_gather_best(pcabo_comm* comm, const double* local, int n_local, double* all);
int pcabo_comm_last_error(pcabo_comm* comm, char* buf, int buflen);
int pcabo_comm_destroy(pcabo_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* PCABO_H */
