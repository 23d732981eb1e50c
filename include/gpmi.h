/*
 * gpmi.h — C-ABI of the MI355X-native Gaussian-process regression hot path.
 *
 * Drop-in boundary for the `inference.gp` path of C-bowman/inference-tools
 * (reference @ 2025-06-14).  The reference is pure Python and has NO FFI of its
 * own; each entry point below therefore cites the
 * reference *Python* function it replaces (file:line relative to the reference
 * root).  The Python host package `inference_amd` binds these through ctypes
 * (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain C: opaque handle, raw pointers, 64-bit sizes; no torch / numpy types.
 *   - all arithmetic is IEEE fp64; matrices are row-major (NumPy C order).
 *   - pointers named *_host are host memory owned by the caller; the library
 *     owns every device buffer behind the handle.  Pointers named *_dev in the
 *     `gpmi_dev_*` block are device pointers (tests / micro-benchmarks).
 *   - every function returns an int status: 0 = ok, <0 = error
 *     (GPMI_ERR_*; text via gpmi_last_error).  Numerical failure of the
 *     Cholesky factorisation is NOT an error status: it is reported LAPACK-style
 *     through `info` (0 = ok, k>0 = leading minor of order k is not positive
 *     definite / not finite), which the host maps to the reference's
 *     `LinAlgError` handling (regression.py:536-542).
 *   - calls on one handle are serialised on the handle's HIP stream; several
 *     handles may be used concurrently from different threads / on different
 *     devices.  No callbacks into the caller.
 */
#ifndef GPMI_H
#define GPMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPMI_VERSION 100

/* covariance kernels (covariance.py:181-279 SquaredExponential, 282-368 RationalQuadratic) */
#define GPMI_KERNEL_SE 0 /* theta = [ln a, ln l_1..ln l_d]            n_theta = d+1 */
#define GPMI_KERNEL_RQ 1 /* theta = [ln a, ln kappa, ln l_1..ln l_d]  n_theta = d+2 */
/* Matern kernels of order 3/2 and 5/2 (no counterpart in the reference), theta laid out as for SE.  With
 * t = sqrt(2 nu sum_k ((u_k - v_k) / l_k)^2):  K = a^2 (1 + t) e^-t  and  K = a^2 (1 + t + t^2 / 3) e^-t. */
#define GPMI_KERNEL_M32 3 /* theta = [ln a, ln l_1..ln l_d]            n_theta = d+1 */
#define GPMI_KERNEL_M52 4 /* theta = [ln a, ln l_1..ln l_d]            n_theta = d+1 */
/* sum of 2..4 SE / RQ / Matern kernels (CompositeCovariance, covariance.py:33-36,47-105) declared per handle by gpmi_set_sum:
 * theta = the components' own parameter vectors back to back, in component order; n_theta = the sum of theirs.
 * Accepted by gpmi_fit, gpmi_lml, gpmi_lml_batch(_submit), gpmi_lml_grad(_batch), gpmi_loo_terms, gpmi_loo_grad(_batch),
 * gpmi_covariance, gpmi_cross_covariance; a sum fit serves gpmi_predict, gpmi_posterior, gpmi_get_K, gpmi_get_L and
 * gpmi_append_point.  Every other entry point returns GPMI_ERR_ARG for it. */
#define GPMI_KERNEL_SUM 2
/* Periodic kernel (no counterpart in the reference; scikit-learn's ExpSineSquared, GPy's StdPeriodic): periodic in the
 * input dimensions declared per handle by gpmi_set_periodic, squared-exponential in the others,
 *   K = a^2 exp(-sum_k w_k / l_k^2),   w_k = 1/2 dx_k^2 (plain k)   or   2 sin^2(pi dx_k / p_k) (periodic k);
 * theta = [ln a, ln l_1..ln l_d, ln p_j for the declared dimensions j in ascending order], n_theta = 1 + d + n_per.
 * d + n_per <= 64: the periods travel in the unused part of the 64 length-scale slots of a parameter block.
 * Accepted wherever GPMI_KERNEL_SE is by the entry points that take a kernel id through gpmi_fit's argument checks
 * (gpmi_fit, gpmi_lml, gpmi_lml_batch(_submit), gpmi_lml_grad(_batch)(_noise), gpmi_loo_terms, gpmi_loo_grad(_batch)(_noise),
 * gpmi_predict(_batch), gpmi_posterior(_draws), gpmi_covariance, gpmi_cross_covariance, gpmi_append_point,
 * gpmi_spatial_derivatives, gpmi_gradient) and as a component of gpmi_set_sum.  GPMI_ERR_ARG, before anything is
 * launched, from gpmi_lml_hessian, gpmi_sgp_*, gpmi_select_points, gpmi_mt_*, gpmi_ggp_*, gpmi_linv_* and the *_mix entry
 * points. */
#define GPMI_KERNEL_PER 5
#define GPMI_MAX_PERIODIC 8 /* periodic dimensions of one handle */

#define GPMI_OK 0
#define GPMI_ERR_ARG (-1)     /* bad argument / call order */
#define GPMI_ERR_HIP (-2)     /* HIP runtime error */
#define GPMI_ERR_NOMEM (-3)   /* device allocation failed */
#define GPMI_ERR_NODEVICE (-4)/* no usable gfx950 device */
#define GPMI_ERR_INTERNAL (-5) /* internal consistency check failed (a bug: please report) */

typedef struct gpmi_ctx gpmi_ctx;

/* ---- lifecycle ------------------------------------------------------------------ */
int gpmi_version(void);
/* number of visible HIP devices (does not create a context) */
int gpmi_device_count(int* count);
/* PCI bus id ("0000:c1:00.0") of visible device `device` into buf (cap >= 16 bytes, NUL-terminated): a physical identity
 * that does not depend on HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES, used by the sharded drivers to tell whether two
 * ranks share a device (no reference counterpart: regression.py:597-601 farms its work over CPU processes) */
int gpmi_device_pci_bus_id(int device, char* buf, int cap);
/* create a handle bound to `device` (own stream + workspaces) */
int gpmi_create(int device, gpmi_ctx** ctx);
int gpmi_destroy(gpmi_ctx* ctx);
/* text of the last error on this handle (ctx may be NULL: last create error) */
const char* gpmi_last_error(const gpmi_ctx* ctx);
/* block until all work queued on the handle's stream has finished */
int gpmi_sync(gpmi_ctx* ctx);
/* bytes the library holds at this moment, over every handle and object of the process: out[0] device memory, out[1]
 * pinned host memory.  Takes no handle and makes no HIP call (two counters kept where the library allocates and frees);
 * what gpmi_destroy returns to the totals is what the handle had taken. */
int gpmi_live_bytes(int64_t out[2]);

/* ---- data -------------------------------------------------------------------------
 * Replaces GpRegressor.__init__ storing x, y and sig (regression.py:94-133, 246-322) and
 * CovarianceFunction.pass_spatial_data (covariance.py:212-226, 309-321): only x (n x d),
 * y (n) and the data-error covariance are uploaded — the N x N x d tensors of the
 * reference are never formed.
 *   noise_var_host : n values y_err**2 (regression.py:320) or NULL for zeros (regression.py:322)
 *   y_cov_host     : dense n x n y-covariance (regression.py:262-293) or NULL; replaces noise_var
 * Limit: 1 <= d <= 64 spatial dimensions (the reference has no such limit).  The covariance kernels stage two
 * [d][64] point panels in LDS - 64 KiB at d = 64 - and carry the d length scales by value.  A larger d returns
 * GPMI_ERR_ARG with a message that names the limit, before anything is released: the handle keeps the data set and
 * the fit it had and takes the next gpmi_set_data.
 */
int gpmi_set_data(gpmi_ctx* ctx, const double* x_host, const double* y_host,
                  const double* noise_var_host, const double* y_cov_host, int64_t n, int64_t d);

/* ---- fit ---------------------------------------------------------------------------
 * Replaces GpRegressor.set_hyperparameters (regression.py:218-244):
 *   K_xx = K(theta) + extra_diag*I + sig ; L = chol(K_xx) ; alpha = L^-T L^-1 (y - mu)
 *   theta_host  : covariance hyper-parameters (log space), n_theta values
 *   extra_diag  : variance added to the diagonal by a `+ WhiteNoise()` component
 *                 (covariance.py:163-169), 0 otherwise
 *   mu_host     : the mean vector MeanFunction.build_mean(theta_mean) (mean.py:47-48), n values
 *   alpha_host  : out, n values          logdet_host : out, sum_i ln L_ii
 * The factor stays resident on the device for predict / posterior / gradients.
 */
int gpmi_fit(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
             const double* mu_host, double* alpha_host, double* logdet_host, int* info);

/* ---- log-marginal likelihood ------------------------------------------------------
 * Replaces GpRegressor.marginal_likelihood (regression.py:528-542):
 *   lml = -1/2 |L^-1 (y-mu)|^2 - sum ln L_ii      (no -(n/2) ln 2 pi term, as the reference)
 * Uses a scratch matrix: the fitted state of gpmi_fit is not disturbed.
 * If info != 0 the value written is -1e50 (regression.py:540-542 sentinel; the host warns).
 */
int gpmi_lml(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
             const double* mu_host, double* lml_host, int* info);

/* T independent evaluations of gpmi_lml (hyper-parameter grid / DE population / PT chains):
 *   thetas_host : T x n_theta      extra_diag_host : T values or NULL
 *   mus_host    : T x n mean vectors, or NULL with mu_const_host : T constants (ConstantMean)
 *   lml_host    : T out            info_host : T out
 * Evaluations are spread over the handle's worker streams (gpmi_set_streams). */
int gpmi_lml_batch(gpmi_ctx* ctx, int kernel, int64_t T, const double* thetas_host, int n_theta,
                   const double* extra_diag_host, const double* mus_host,
                   const double* mu_const_host, double* lml_host, int* info_host);
/* Asynchronous form of gpmi_lml_batch for the lockstep sizes (n <= 4096, diagonal data errors): submit enqueues the T
 * (<= 256; GPMI_ASYNC_SLOT_MAX) evaluations of slot 0 or 1 and returns at once, wait blocks until they are through and delivers lml[T] /
 * info[T] in the order submitted.  The two slots are the two halves of the lockstep workspace and run side by side; a
 * value is bit-identical to what gpmi_lml_batch returns for the same hyper-parameters.  What it is for: a tempering
 * driver (mcmc/parallel.py:190-231 in the reference: one process per chain, results over pipes) splits its ladders
 * in two groups and does the accept / reject bookkeeping of one group while the device evaluates the other.
 * While a slot is pending, gpmi_lml_batch / gpmi_lml_grad_batch on the same handle are refused (GPMI_ERR_ARG). */
int gpmi_lml_batch_submit(gpmi_ctx* ctx, int kernel, int64_t T, const double* thetas_host, int n_theta,
                          const double* extra_diag, const double* mus_host, const double* mu_const, int slot);
int gpmi_lml_batch_wait(gpmi_ctx* ctx, int slot, double* lml, int* info);

/* number of concurrent worker streams (each with its own n x n scratch) used by gpmi_lml_batch */
int gpmi_set_streams(gpmi_ctx* ctx, int n_streams);
/* Handle options.
 *   GPMI_OPT_LOCKSTEP_ALWAYS  1: gpmi_lml_batch / gpmi_lml take the lockstep path (all evaluations of a call in one
 *       launch sequence, batch in blockIdx.z) for ANY number of evaluations while n <= 4096, also for T = 1.  A
 *       value then does not depend on which other evaluations share its call - what the lockstep MCMC drivers
 *       (GibbsChain retries make the batches ragged, reference gibbs.py:635-648) need for trajectories that are
 *       bit-identical however the chains are grouped.  0 (default): a single evaluation uses the lane path. */
#define GPMI_OPT_LOCKSTEP_ALWAYS 1
/*   GPMI_OPT_RESERVE_POINTS   r >= 0, read by the NEXT gpmi_set_data: room for r more training points in the padded
 *       device matrices (identity in the padding: the factor is unaffected), to be filled by gpmi_append_point */
#define GPMI_OPT_RESERVE_POINTS 2
/*   GPMI_OPT_NO_FLOW          1: factorisations of this handle keep the stream-ordered schedule for their chain-bound
 *     part instead of the flag-ordered tile-task launch (same factor, bit for bit; slower).  The flag-ordered launch
 *     needs its two kernels side by side on the device; when something outside the library prevents that for about
 *     a second (a heavily oversubscribed device, a tool that serialises kernels) the call fails with
 *     GPMI_ERR_INTERNAL instead of hanging - a caller can then set this option and repeat the call (the Python layer
 *     does, once, with a warning). */
#define GPMI_OPT_NO_FLOW 3
int gpmi_set_option(gpmi_ctx* ctx, int option, int value);

/* Allocate now what gpmi_lml_grad would allocate inside its first call - the evaluation lane (a second n x n matrix,
 * its streams), the matrix of L^-T, the contraction's partial sums for n_theta covariance parameters - so that the first
 * gradient evaluation of an optimiser run costs what the others cost (N = 16384: 169 ms -> 78 ms; the reference has no
 * counterpart: regression.py:544-567 allocates its N x N temporaries in every call). */
int gpmi_prepare_gradient(gpmi_ctx* ctx, int n_theta);

/* Replaces GpRegressor.marginal_likelihood_gradient (regression.py:544-567):
 *   grad_theta_host : n_theta values  1/2 sum (alpha alpha^T - K^-1) o dK/dtheta_j
 *                     (dK_j recomputed from x on the fly: covariance.py:268-276, 350-365)
 *   trace_q_host    : sum_i (alpha_i^2 - K^-1_ii)  (= d/d extra_diag * 2; WhiteNoise gradient,
 *                     covariance.py:171-175) or NULL
 *   alpha_host      : n values K^-1 (y-mu) for the mean-parameter gradients (regression.py:563)
 * No sentinel here: info != 0 is returned to the host, which raises like the reference
 * (regression.py:555 has no LinAlgError guard). */
int gpmi_lml_grad(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta,
                  double extra_diag, const double* mu_host, double* lml_host,
                  double* grad_theta_host, double* trace_q_host, double* alpha_host, int* info);
/* T evaluations of gpmi_lml_grad (marginal_likelihood_gradient, regression.py:544-567) in one call - the L-BFGS-B starts
 * of the hyper-parameter search (regression.py:585-605: the reference farms them over a multiprocessing.Pool).  For
 * padded N <= 4096 the evaluations of a chunk advance in LOCKSTEP (every launch carries the chunk, as in
 * gpmi_lml_batch); larger problems run one after another.  thetas: T x n_theta; extra, mu_const: T (or mus: T x n);
 * outputs lml (T), grad_theta (T x n_theta), trace_q (T, may be NULL), alpha_host (T x n, may be NULL), info (T). */
int gpmi_lml_grad_batch(gpmi_ctx* ctx, int kernel, int64_t T, const double* thetas_host, int n_theta,
                        const double* extra_diag_host, const double* mus_host, const double* mu_const_host,
                        double* lml, double* grad_theta, double* trace_q, double* alpha_host, int* info);

/* The log-marginal likelihood, its gradient and its exact Hessian from one factorisation (an addition: the reference has
 * no second derivatives).  With D_i = dK / d theta_i, D_ij the second derivatives, G_i = K^-1 D_i, z_i = G_i alpha,
 * Q = alpha alpha^T - K^-1 and the prior mean mu = Phi^T m (every mean function of the package is linear):
 *   H_ij       = 1/2 sum_ab Q_ab (D_ij)_ab - (D_i alpha)^T z_j + 1/2 tr(G_i G_j)     (two covariance parameters)
 *   H_{m_p m_q} = -phi_p^T K^-1 phi_q,       H_{m_p theta_j} = -phi_p^T z_j
 * of LML = -1/2 r^T alpha - sum ln L_ii (no 2 pi term, as gpmi_lml).  Derivatives by ln a act on the a^2 part of K, its
 * a^2 1e-12 jitter included, and not on the noise.
 *   mu_host   : n prior means at theta's mean parameters;   phi_host : n_mean x n rows d mu / d m_p, or NULL with n_mean = 0
 *   grad_host : n_theta + 1 values - the kernel's parameters, then ln sigma of extra_diag = sigma^2
 *   hess_host : (n_mean + n_theta + 1)^2 values, row-major; rows and columns: the mean's parameters, the kernel's, ln sigma
 * With extra_diag = 0 the last row and column and the last entry of grad_host are zeros.  The matrix is symmetric bit for
 * bit (i <= j is computed, then mirrored), a repeated call returns the same bits (no atomics, every sum in an order fixed
 * by n, d and the kernel), and so does a call that splits the parameters into groups (below).
 * Kernels: GPMI_KERNEL_SE, _RQ, _M32, _M52.  GPMI_ERR_ARG with a message, before anything is launched: GPMI_KERNEL_SUM or a
 * handle with gpmi_set_sum, a dense y covariance, a NULL pointer that is not optional, n_mean outside 0 .. 1 + 2 x 64.
 * (Per-point noise variances that are hyper-parameters - gpmi_set_noise - have derivatives this entry point does not
 * form: the caller differences gpmi_lml_grad for them.)  A matrix that does not factorise: info > 0, the outputs are
 * untouched, GPMI_OK.  Runs on lane 1 like gpmi_lml_grad: the fitted state of gpmi_fit is not touched.
 * Workspace: the handle's own buffers, freed with it - per parameter of a group the n x n matrices D_i and G_i.  The
 * n_theta + 1 parameters form ONE group when 3 (n_theta + 1) padded matrices fit GPMI_HESS_GIB (environment, GiB,
 * fractions allowed, 0 < v <= 200, default 24; read at every call), else groups of floor(cap / (3 matrices)) parameters,
 * with a third set of matrices for the G_j of the group a group is paired with; when not even one parameter fits:
 * GPMI_ERR_ARG.  (A padded matrix: np x (np + 32) doubles, np = n rounded up to 128 plus the reserve.)
 * Profile classes (they share the ids of the sparse model's stages, which a GpRegressor handle does not run):
 * GPMI_PROF_HESS_BUILD - the D_i and D_i alpha; _GEMM - the products G_i and z_i; _TRACE - the pair traces;
 * _CONTRACT - the second-derivative contraction. */
int gpmi_lml_hessian(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
                     const double* mu_host, const double* phi_host, int n_mean, double* lml_host, double* grad_host,
                     double* hess_host, int* info);
/* alpha = K^-1 (y - mu) of the last gpmi_lml_hessian (or gpmi_lml_grad) on this handle, n values: the gradient by the
 * mean's parameters is Phi alpha. */
int gpmi_lml_hessian_alpha(gpmi_ctx* ctx, double* alpha_host);

/* ---- prediction (needs a prior gpmi_fit) --------------------------------------------
 * Replaces the per-point loop of GpRegressor.__call__ (regression.py:188-216) by one batched
 * cross-covariance + triangular solve:
 *   mu_host[m]  = k(q_m, x) . alpha            (the host adds MeanFunction(q), regression.py:212)
 *   var_host[m] = a^2 - |L^-1 k(q_m, x)|^2     (the host takes sqrt(abs(.)), regression.py:216)
 */
int gpmi_predict(gpmi_ctx* ctx, const double* pts_host, int64_t m, double* mu_host,
                 double* var_host);
/* Prediction under T hyper-parameter vectors at once, and its mixture (an addition: the reference predicts under one
 * fitted theta).  For row t of thetas, gpmi_predict's values after a gpmi_fit at that row:
 *   mean_t[t][q] = k_t(q, x) . alpha_t + mu_q[t][q]   (mu_q NULL: + mu_const[t])
 *   var_t[t][q]  = | a_t^2 - |L_t^-1 k_t(x, q)|^2 |   (the square of the reference's sqrt(abs(.)), regression.py:216)
 * and over the rows that factorised, with weights w_t (weights_host NULL: equal), in two passes (law of total variance):
 *   mix_mean[q] = sum_t w_t mean_t[t][q],   mix_var[q] = sum_t w_t (var_t[t][q] + (mean_t[t][q] - mix_mean[q])^2).
 * thetas / extra / mus | mu_const as gpmi_lml_grad_batch; pts: m x d; weights: T finite values >= 0 with a positive sum.
 * mean_t, var_t (T x m) and mix_mean, mix_var (m) may each be NULL; with var_t and mix_var both NULL no variance is
 * computed.  A row that does not factorise gets info[t] != 0 and NaN in mean_t / var_t and is left out of the mixture:
 * the other rows' weights are divided by their sum (equal weights: 1 / number of good rows); no good row: NaN mixtures,
 * GPMI_OK.  Lockstep sizes only (padded n <= 4096, diagonal data errors; SE, RQ, Matern, GPMI_KERNEL_SUM): every launch carries
 * a chunk of rows, also for T = 1, so a row's values do not depend on the batch it is in; the sums over t run as a
 * pairwise tree over the good rows in order, so they depend on T and the failures alone.  The points are processed in
 * panels of GPMI_PREDICT_PANEL rows.  The fitted state of gpmi_fit is not touched. */
#define GPMI_PREDICT_PANEL 256
int gpmi_predict_batch(gpmi_ctx* ctx, int kernel, int64_t T, const double* thetas_host, int n_theta,
                       const double* extra_diag_host, const double* mus_host, const double* mu_const_host,
                       const double* pts_host, int64_t m, const double* mu_q_host, const double* weights_host,
                       double* mean_t_host, double* var_t_host, double* mix_mean_host, double* mix_var_host, int* info);
/* Replaces GpRegressor.build_posterior (regression.py:421-449): mu (m) and
 * Sigma = K_qq - Q^T Q (m x m), Q = L^-1 K_qx^T.  cov_host may be NULL (mean_only). */
int gpmi_posterior(gpmi_ctx* ctx, const double* pts_host, int64_t m, double* mu_host,
                   double* cov_host);
/* Replaces GpRegressor.spatial_derivatives (regression.py:387-419), SE and the Matern kernels only
 * (RationalQuadratic has no gradient_terms: covariance.py:38-44; sums and mixtures are refused): dmu (m x d), dvar (m x d). */
int gpmi_spatial_derivatives(gpmi_ctx* ctx, const double* pts_host, int64_t m, double* dmu_host,
                             double* dvar_host);
/* Replaces GpRegressor.gradient (regression.py:351-385), SE and the Matern kernels only: mean (m x d) and covariance
 * (m x d x d) of the gradient of the regression estimate. */
int gpmi_gradient(gpmi_ctx* ctx, const double* pts_host, int64_t m, double* gmu_host,
                  double* gcov_host);

/* Replaces GpRegressor.loo_likelihood_gradient (regression.py:489-526): besides alpha and diag(K^-1)
 * returns p = K^-1 (alpha / diag) (for the mean-parameter gradients, regression.py:516-520) and
 *   grad_theta_host[j] = sum_ab dK_j[a][b] (sym(p alpha^T) - K^-1 diag(c2) K^-1)_ab   (regression.py:511-514)
 *   trace_q_host       = trace of that matrix (WhiteNoise gradient = 2 sigma^2 trace).
 * No sentinel: info != 0 makes the host raise, as regression.py:501 has no LinAlgError guard. */
int gpmi_loo_grad(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
                  const double* mu_host, double* alpha_host, double* ikdiag_host, double* p_host,
                  double* grad_theta_host, double* trace_q_host, int* info);
/* gpmi_lml_grad_batch with noise variances of their own for every evaluation (noise_var_host: T x n) and the diagonal of
 * alpha alpha^T - K^-1 back (qdiag_host: T x n): what HeteroscedasticNoise (covariance.py:608-690: one variance per point IS
 * a hyper-parameter, its gradient is exp(2 theta_i) qdiag_i, :683-689) needs from a batch - the single-evaluation form is
 * gpmi_set_noise + gpmi_lml_grad + gpmi_lml_grad_qdiag. */
int gpmi_lml_grad_batch_noise(gpmi_ctx* ctx, int kernel, int64_t T, const double* thetas_host, int n_theta,
                              const double* extra_diag_host, const double* mus_host, const double* mu_const_host,
                              const double* noise_var_host, double* lml_host, double* grad_theta_host,
                              double* trace_q_host, double* alpha_host, double* qdiag_host, int* info);

/* The same for T hyper-parameter vectors at once (thetas: T x n_theta, extra / mu_const: T values or mus: T x n; outputs
 * T x n, T x n_theta, T): for n <= 4096 every launch carries the whole chunk (lockstep, like gpmi_lml_grad_batch); the
 * multi-start search with the cross-validation objective (regression.py:159-164, 585-605) advances all its starts on it. */
int gpmi_loo_grad_batch(gpmi_ctx* ctx, int kernel, int64_t T, const double* thetas_host, int n_theta,
                        const double* extra_diag_host, const double* mus_host, const double* mu_const_host,
                        double* alpha_host, double* ikdiag_host, double* p_host, double* grad_theta_host,
                        double* trace_q_host, int* info);
/* gpmi_loo_grad_batch with noise variances of their own for every evaluation (noise_var_host: T x n) and, back, the diagonal of
 * M = K^-1 diag(c2) K^-1 (mdiag_host: T x n): the leave-one-out gradient with respect to HeteroscedasticNoise's parameter of
 * point i is 2 exp(2 theta_i) (p_i alpha_i - M_ii) (regression.py:509-514 with dK = 2 s_i^2 e_i e_i^T, covariance.py:683-689).
 * Lockstep sizes only (n <= 4096, diagonal data errors); the cross_val = True search of such a model advances its starts on it. */
int gpmi_loo_grad_batch_noise(gpmi_ctx* ctx, int kernel, int64_t T, const double* thetas_host, int n_theta,
                              const double* extra_diag_host, const double* mus_host, const double* mu_const_host,
                              const double* noise_var_host, double* alpha_host, double* ikdiag_host, double* p_host,
                              double* mdiag_host, double* grad_theta_host, double* trace_q_host, int* info);

/* ---- covariance plugin surface -----------------------------------------------------
 * Replaces CovarianceFunction.build_covariance (covariance.py:247-255, 343-348): the n x n matrix
 * a^2 (C + 1e-12 I) + extra_diag I, plus the data-error covariance when with_noise != 0. */
int gpmi_covariance(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta,
                    double extra_diag, int with_noise, double* K_host);
/* Replaces CovarianceFunction.__call__(u, v = x, theta) (covariance.py:240-245, 335-341):
 * the m x n cross-covariance between pts and the stored x, no jitter. */
int gpmi_cross_covariance(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta,
                          const double* pts_host, int64_t m, double* out_host);

/* ---- lazy attribute downloads (GpRegressor.K_xx / .L, regression.py:239-241) ------- */
int gpmi_get_K(gpmi_ctx* ctx, double* K_host); /* n x n, rebuilt from the fitted theta */
int gpmi_get_L(gpmi_ctx* ctx, double* L_host); /* n x n lower factor, upper triangle zero */

/* ---- leave-one-out (regression.py:451-526) ------------------------------------------ */
/* diag(K^-1) of the fitted model: var = 1/diag, mu = y - alpha*var on the host (regression.py:460-466) */
int gpmi_loo_diag(gpmi_ctx* ctx, double* ikdiag_host);
/* alpha = K^-1 (y - mu) and diag(K^-1) at an arbitrary theta (scratch matrix; the fitted state is not
 * disturbed): the O(n^3) part of GpRegressor.loo_likelihood (regression.py:468-487); the host forms
 * -1/2 sum(var alpha^2 + ln var), var = 1/diag.  info != 0 -> the host returns the -1e50 sentinel. */
int gpmi_loo_terms(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta,
                   double extra_diag, const double* mu_host, double* alpha_host,
                   double* ikdiag_host, int* info);

/* ---- per-point noise hyper-parameters (HeteroscedasticNoise, covariance.py:608-690) ----
 * K = K_stationary + diag(sigma_i^2) + data errors: the host adds exp(2 theta_i) to the data variances and
 * replaces the diagonal term with this call before gpmi_fit / gpmi_lml / gpmi_lml_grad (n values; ignored
 * when a dense y_cov was given to gpmi_set_data). */
int gpmi_set_noise(gpmi_ctx* ctx, const double* noise_var_host);

/* ---- sums of stationary kernels (GPMI_KERNEL_SUM) ------------------------------------
 * Declares the components of the handle's sum: nk in 2..4, kernels[m] GPMI_KERNEL_SE, _RQ, _M32, _M52 or _PER in the order of
 * the sum.  K = sum_m a_m^2 (C_m + 1e-12 I) + extra_diag I + data errors (every component carries its own jitter,
 * covariance.py:254-255,348); a query point's prior variance is sum_m a_m^2. */
int gpmi_set_sum(gpmi_ctx* ctx, int nk, const int* kernels);
/* ---- periodic dimensions (GPMI_KERNEL_PER) ---------------------------------------------
 * Declares the input dimensions in which the handle's GPMI_KERNEL_PER is periodic: n_per in 1..GPMI_MAX_PERIODIC,
 * dims[n_per] strictly ascending, each in [0, d).  Called after gpmi_set_data; the declaration is kept until a
 * gpmi_set_data with another d.  Every GPMI_KERNEL_PER component of a sum shares it.  GPMI_ERR_ARG with a message (the
 * handle stays usable, an earlier declaration stays in force): NULL dims, n_per out of range, dims not strictly
 * ascending, a dim >= d, no data set.  GPMI_KERNEL_PER itself is GPMI_ERR_ARG until a declaration exists. */
int gpmi_set_periodic(gpmi_ctx* ctx, int n_per, const int* dims);
/* q_i = alpha_i^2 - (K^-1)_ii of the most recent gpmi_lml_grad call (n values): the gradient with respect to
 * ln sigma_i is 1/2 Q_ii 2 sigma_i^2 = sigma_i^2 q_i (covariance.py:682-686, regression.py:561-565). */
int gpmi_lml_grad_qdiag(gpmi_ctx* ctx, double* qdiag_host);

/* ---- mixture covariance: ChangePoint (covariance.py:371-606) ---------------------------
 * K = sum_m diag(g_m) K_m(theta_m) diag(g_m) + extra_diag I + data errors, with up to four stationary
 * sub-kernels K_m and per-point weights g_m (products of the logistic windows of covariance.py:529-559,
 * evaluated on the host in O(N)).  kernels[nk]: GPMI_KERNEL_*; thetas: the sub-kernels' parameter vectors
 * concatenated; n_thetas[nk]; g_host: nk x n row-major. */
int gpmi_fit_mix(gpmi_ctx* ctx, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                 const double* g_host, double extra_diag, const double* mu_host, double* alpha_host,
                 double* logdet, int* info);
int gpmi_lml_mix(gpmi_ctx* ctx, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                 const double* g_host, double extra_diag, const double* mu_host, double* lml, int* info);
/* LML and the gradient pieces (covariance.py:561-594 + regression.py:544-567): grad_thetas = the sub-kernels'
 * parameter gradients, concatenated; hrows: the window row sums, Q = alpha alpha^T - K^-1, from which the host forms the
 * window-parameter gradients.  hw_host == NULL: hrows is nk x n, h_m(i) = sum_j Q_ij K_m,ij g_m(j) (two regions: the host
 * contracts sum_i dw_i (h_1 - h_0)_i).  hw_host != NULL (nk x 2 x n, round 5): the caller's own row-sum weights, two per
 * sub-kernel, hrows nk x 2 x n with h_{m,r}(i) = sum_j Q_ij K_m,ij hw_{m,r}(j) - covariance.py:588-593 differentiates
 * change-point c through the factors (1 - f_c) of K_c and f_c of K_{c+1} ONLY, whatever other windows multiply them, so
 * for any number of regions the host passes hw_{m,0} = f_{m-1}, hw_{m,1} = 1 - f_m and contracts
 * sum_i df_c(i) (h_{c+1,0} - h_{c,1})(i); the same expression as hw == NULL when nk = 2.
 * q_i for additive noise terms comes from gpmi_lml_grad_qdiag as usual. */
int gpmi_lml_grad_mix(gpmi_ctx* ctx, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                      const double* g_host, const double* hw_host, double extra_diag, const double* mu_host, double* lml,
                      double* grad_thetas, double* hrows_host, double* alpha_host, int* info);

/* gpmi_lml_grad_mix for T hyper-parameter vectors in one call (round 4; regression.py:544-567 with a ChangePoint kernel,
 * covariance.py:529-594, for the T starts of multistart_bfgs, regression.py:585-605).  N <= 4096: the evaluations advance
 * in lockstep, every launch carrying all of them.  thetas: T rows, each the sub-kernels' parameters back to back
 * (sum of n_thetas values); g: T x nk x n window weights; hw: NULL or T x nk x 2 x n row-sum weights (see
 * gpmi_lml_grad_mix); extra: T WhiteNoise variances (or NULL); one of mus (T x n) / mu_const (T).  Out: lml[T],
 * grad_thetas[T x sum n_thetas], hrows[T x nk x n] (hw == NULL: h_m(i) = sum_j Q_ij K_m,ij g_m(j)) or [T x nk x 2 x n],
 * optional alpha_out[T x n], qdiag_out[T x n] (diag(alpha alpha^T - K^-1)), info[T]. */
int gpmi_lml_grad_batch_mix(gpmi_ctx* ctx, int nk, const int* kernels, int64_t T, const double* thetas,
                            const int* n_thetas, const double* g, const double* hw, const double* extra,
                            const double* mus, const double* mu_const, double* lml, double* grad_thetas, double* hrows,
                            double* alpha_out, double* qdiag_out, int* info);
/* The leave-one-out counterpart (regression.py:489-526 with covariance.py:529-594) for T hyper-parameter vectors in lockstep:
 * alpha, diag(K^-1), p = K^-1 (alpha / diag) and diag(M), M = K^-1 diag(c2) K^-1, per evaluation (T x n each); the
 * sub-kernels' gradient components (T x sum n_thetas) and the window row sums h_m(i) = sum_j (sym(p alpha^T) - M)_ij K_m,ij g_m(j)
 * (T x nk x n; window parameters: 2 sum_i dw_i (h_1 - h_0)_i on the host; WhiteNoise: 2 s^2 sum(p o alpha - diag M)); with
 * hw_host (T x nk x 2 x n, see gpmi_lml_grad_mix) the row sums use the caller's weights, T x nk x 2 x n: any number of regions.
 * Lockstep sizes only (n <= 4096, diagonal data errors). */
int gpmi_loo_grad_batch_mix(gpmi_ctx* ctx, int nk, const int* kernels, int64_t T, const double* thetas_host,
                            const int* n_thetas, const double* g_host, const double* hw_host,
                            const double* extra_diag_host, const double* mus_host, const double* mu_const_host,
                            double* alpha_host, double* ikdiag_host, double* p_host, double* mdiag_host,
                            double* grad_thetas_host, double* hrows_host, int* info);
/* alpha and diag(K^-1) at arbitrary hyper-parameters: the O(n^3) part of loo_likelihood (regression.py:468-487) */
int gpmi_loo_terms_mix(gpmi_ctx* ctx, int nk, const int* kernels, const double* thetas, const int* n_thetas,
                       const double* g_host, double extra_diag, const double* mu_host, double* alpha_host,
                       double* ikdiag_host, int* info);
/* prediction with the model of gpmi_fit_mix: gq_host (nk x m) are the weights of the query points;
 * mu* = k.alpha (the host adds the mean function), negsumsq = -|L^-1 k|^2 (the host adds K_qq[0, 0]) */
int gpmi_predict_mix(gpmi_ctx* ctx, const double* pts_host, int64_t m, const double* gq_host,
                     double* mu_host, double* negsumsq_host);
/* build_posterior (regression.py:421-449) with the model of gpmi_fit_mix: mu = K_qx alpha, cov = K_qq - Q^T Q */
int gpmi_posterior_mix(gpmi_ctx* ctx, const double* pts_host, int64_t m, const double* gq_host,
                       double* mu_host, double* cov_host);

/* ---- Gaussian-process linear inversion (inference/gp/inversion.py) --------------------
 * The model parameters (n of them, at the positions given to gpmi_set_data as x; y / noise of that call are
 * unused) have the GP prior N(mu, K(theta)); the data y (m values, independent errors y_err) are
 * A mu_true + noise with the m x n model matrix A (row-major).  All entry points work on
 * J = A K A^T + diag(y_err^2) = L L^T (inversion.py:189, 198) with the same kernels as the regression path. */
int gpmi_linv_set(gpmi_ctx* ctx, const double* A_host, int64_t m, const double* y_host,
                  const double* y_err_host);
/* Replaces GpLinearInverter.marginal_likelihood (inversion.py:177-191): -1/2 |L^-1 (y - A mu)|^2 - sum ln L_ii */
int gpmi_linv_lml(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
                  const double* mu_host, double* lml, int* info);
/* Replaces GpLinearInverter.marginal_likelihood_gradient (inversion.py:193-217).  grad_theta: the n_theta
 * covariance-parameter gradients 1/2 sum (alpha alpha^T - J^-1) o (A dK_j A^T), evaluated as
 * 1/2 sum (w w^T - A^T J^-1 A) o dK_j with w = A^T alpha; trace_q = sum_a (w_a^2 - (A^T J^-1 A)_aa) for an
 * additive WhiteNoise term; at_alpha (n values) = w, from which the host forms the mean-parameter gradients
 * sum_i alpha_i (A dmu_j)_i = w . dmu_j. */
int gpmi_linv_lml_grad(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
                       const double* mu_host, double* lml, double* grad_theta, double* trace_q,
                       double* at_alpha_host, int* info);
/* Replaces GpLinearInverter.calculate_posterior / calculate_posterior_mean (inversion.py:138-175):
 * mean = mu + K A^T J^-1 (y - A mu), cov = K - K A^T J^-1 A K (the Woodbury form of the reference's
 * solve(I + K A^T Sigma^-1 A, K)); cov_host may be NULL. */
int gpmi_linv_posterior(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta,
                        double extra_diag, const double* mu_host, double* mean_host, double* cov_host,
                        int* info);
/* The same three with a prior covariance the CALLER evaluated (K_host: n x n, row-major, symmetric) - any
 * CovarianceFunction object the reference accepts as `prior_covariance_function` (inversion.py:117-127, plugin ABC
 * covariance.py:8-44): the host calls the object's own build_covariance / covariance_and_gradients, the device does
 * A K A^T + Sigma, the factorisation, the solves and the inverse.  gpmi_linv_lml_grad_dense returns
 * G = A^T J^-1 A (n x n) and w = A^T alpha (at_alpha_host, n): grad_j = 1/2 sum (w w^T - G) o dK_j on the host
 * (inversion.py:202-216 with Q = alpha alpha^T - J^-1 folded through A). */
int gpmi_linv_lml_dense(gpmi_ctx* ctx, const double* K_host, const double* mu_host, double* lml, int* info);
int gpmi_linv_lml_grad_dense(gpmi_ctx* ctx, const double* K_host, const double* mu_host, double* lml,
                             double* G_host, double* at_alpha_host, int* info);
int gpmi_linv_posterior_dense(gpmi_ctx* ctx, const double* K_host, const double* mu_host, double* mean_host,
                              double* cov_host, int* info);

/* ---- multi-GPU result gather (RCCL over xGMI) ----------------------------------------
 * Replaces the result return of multiprocessing.Pool.map (regression.py:600-601) and the
 * (theta, log-prob) messages of the tempering processes (mcmc/parallel.py:195-201).  One process per
 * GPU.  Rank 0 calls gpmi_comm_unique_id (128 bytes), the caller distributes the id over any host
 * channel, every rank calls gpmi_comm_init, then gpmi_comm_allgather gathers `count` doubles per
 * rank (recv_host: world * count, in rank order).  librccl is loaded on first use.
 * No data-path collective exists: the units (hyper-parameter vectors, optimiser starts, tempering ladders) are
 * independent; the communicator carries the data set once at start-up and a few doubles per unit at the end. */
int gpmi_comm_unique_id(char* id_out_128);
int gpmi_comm_init(gpmi_ctx* ctx, int rank, int world, const char* id_128);
int gpmi_comm_allgather(gpmi_ctx* ctx, const double* send_host, double* recv_host, int64_t count);
/* Start-up distribution of the data set: `count` doubles of rank `root`'s buf_host to every rank's buf_host (one
 * ncclBroadcast).  Replaces the pickling of the whole regressor into every worker process
 * (regression.py:597-601, mcmc/parallel.py:127-136): x, y, y_err are all a rank needs to build its own. */
int gpmi_comm_broadcast(gpmi_ctx* ctx, double* buf_host, int64_t count, int root);
/* The number of ranks RCCL sees in the communicator (ncclCommCount). */
int gpmi_comm_count(gpmi_ctx* ctx, int* ranks);
int gpmi_comm_destroy(gpmi_ctx* ctx);

/* Append ONE training point to the fitted model at unchanged hyper-parameters in O(n^2): the new row of the Cholesky
 * factor is l = L^-1 k(X, x_new), l_nn = sqrt(k_nn - l.l) (one triangular sweep), alpha is re-solved (two sweeps).
 * The reference has no counterpart: GpOptimiser.add_evaluation re-fits from scratch (optimisation.py:177-186,
 * O(n^3) per added point even when the hyper-parameters are kept).  Needs a fit by gpmi_fit (one stationary kernel or a sum of them, diagonal
 * data errors) and free capacity (GPMI_OPT_RESERVE_POINTS).
 *   x_new_host : d values    mu_host : n + 1 prior means (the old points' first)    alpha_host : n + 1 out
 *   info : 0, or n + 1 if the enlarged matrix is not positive definite (the model is then left unchanged) */
int gpmi_append_point(gpmi_ctx* ctx, const double* x_new_host, double y_new, double noise_var_new,
                      const double* mu_host, double* alpha_host, double* logdet_host, int* info);
/* points the handle has room for (n + free capacity) */
int gpmi_capacity(gpmi_ctx* ctx, int64_t* capacity);

/* ---- dense entry points: covariance functions that only implement the plugin ABC -------------------------
 * Reference: CovarianceFunction (inference/gp/covariance.py:8-44) is an open plugin contract and GpRegressor
 * (regression.py:134-155) accepts any object implementing it.  For a kernel the library has no device code for, the
 * host evaluates the plugin's own build_covariance / __call__ and passes the dense matrices; every O(N^3) step
 * (numpy.linalg.cholesky regression.py:241, solve_triangular :242-244 / :213 / :447, the explicit inverse :556-557)
 * runs on the device.  gpmi_set_data must have been called (x is unused, y and n are).
 *   K_host : n x n row-major, the complete K(theta) + Sigma (only its lower triangle is read) */
/* fit (regression.py:218-244) on lane 0; afterwards gpmi_predict_dense / gpmi_solve_rows / gpmi_get_L /
 * gpmi_loo_diag use this factor */
int gpmi_fit_dense(gpmi_ctx* ctx, const double* K_host, const double* mu_host, double* alpha_host,
                   double* logdet_host, int* info);
/* LML (regression.py:528-542) of a dense K on a scratch lane; alpha_host (n) and iK_host (n x n, K^-1, what
 * marginal_likelihood_gradient :555-565 and the LOO expressions :460-526 contract with the plugin's own dK) are
 * optional (NULL) */
int gpmi_lml_dense(gpmi_ctx* ctx, const double* K_host, const double* mu_host, double* lml_host,
                   double* alpha_host, double* iK_host, int* info);
/* leave-one-out pieces (regression.py:468-526) of a dense K on a scratch lane: alpha, diag(K^-1), and for the
 * gradient the two parameter-independent pieces p = K^-1 c1 (n) and W = K^-1 diag(c2) K^-1 (n x n) with
 * c1 = alpha var, c2 = var (1 + var alpha^2) / 2, var = 1 / diag(K^-1): d LOO / d theta_j = p . (dK_j alpha) -
 * sum dK_j o W for the plugin's own dK_j (p_host, W_host may be NULL) */
int gpmi_loo_dense(gpmi_ctx* ctx, const double* K_host, const double* mu_host, double* alpha_host,
                   double* ikdiag_host, double* p_host, double* W_host, int* info);
/* predict pieces (regression.py:208-214) for m query points given their cross-covariances Kq (m x n):
 * kalpha_host[i] = Kq[i] . alpha, sumsq_host[i] = |L^-1 Kq[i]|^2 (either may be NULL) */
int gpmi_predict_dense(gpmi_ctx* ctx, const double* Kq_host, int64_t m, double* kalpha_host, double* sumsq_host);
/* X = Q L^-T for m right-hand sides given as rows (m x n), and / or their Gram matrix X X^T (m x m): the building
 * block of build_posterior (regression.py:447-448) and of gradient / spatial_derivatives (:374-383, :410-417) */
int gpmi_solve_rows(gpmi_ctx* ctx, const double* Q_host, int64_t m, double* X_host, double* gram_host);
/* Z = Q K^-1 = Q L^-T L^-1 for m right-hand sides given as rows (m x n; Z_host m x n), for any fitted model (gpmi_fit or
 * gpmi_fit_dense): the K^-1 k of spatial_derivatives (regression.py:410) with caller-built rows.  The rows are solved in
 * place in chunks of 1024, forward then backward, by the code gpmi_spatial_derivatives runs */
int gpmi_solve_rows_kinv(gpmi_ctx* ctx, const double* Q_host, int64_t m, double* Z_host);

/* ---- kernel-density estimation (GaussianKDE, inference/pdf/kde.py) -------------------
 * A density object holds a sorted sample and its region table on the device; the handle owns it, and gpmi_destroy
 * releases the objects still alive.  Its calls run on a stream of the handle that every density object shares; like every
 * call on a handle they must be serialised by the caller (inference_amd.pdf holds a lock per handle around each one).
 * Replaces GaussianKDE.__init__'s slice table (kde.py:48-90): region r covers the sorted samples [lo_host[r], hi_host[r]),
 * 0 <= lo <= hi <= n. */
typedef struct gpmi_kde gpmi_kde;
int gpmi_kde_create(gpmi_ctx* ctx, int64_t n, const double* sorted_sample_host, int64_t n_regions,
                    const int64_t* lo_host, const int64_t* hi_host, gpmi_kde** out);
/* release a density object (NULL: GPMI_ERR_ARG); not after gpmi_destroy of its handle, which has released it already */
int gpmi_kde_destroy(gpmi_kde* kde);
/* Replaces the slice sums of GaussianKDE.__call__ and .cdf (kde.py:96-133): for the m points x_host[i] of regions
 * region_host[i] (0 <= region < n_regions), over the samples s_j of the region's slice,
 *   pdf_sum_host[i] = sum_j exp(-((x_i - s_j) q)^2),   cdf_sum_host[i] = sum_j (1 + erf((x_i - s_j) q))
 * Either output may be NULL (not both); q is finite and positive.  The caller applies norm, 0.5 / n and the offsets.
 * A point's values do not depend on the other points of the call; repeated calls are bit-identical. */
int gpmi_kde_eval(gpmi_kde* kde, int64_t m, const double* x_host, const int64_t* region_host, double q,
                  double* pdf_sum_host, double* cdf_sum_host);
/* Replaces GaussianKDE.cross_validation_logprob (kde.py:195-218) for n_widths finite, positive bandwidths at once: the
 * leave-one-out log-probability of the n finite samples (any order), with S_i(h) = sum_j exp(-(x_i - x_j)^2 / (2 h^2)),
 *   logprob_host[k] = sum_i [log S_i - log(h_k n sqrt(2 pi)) + log(1 - c / S_i)],   0 < c < 1 */
int gpmi_kde_cv_logprob(gpmi_ctx* ctx, int64_t n, const double* samples_host, int n_widths,
                        const double* widths_host, double c, double* logprob_host);

/* ---- two-dimensional kernel-density estimation (KDE2D, inference/pdf/kde.py:256-280) ----
 * A 2-D density object holds the n finite samples (x_j, y_j) on the device, binned into tiles of nearby samples; the
 * handle owns it (gpmi_destroy releases the objects still alive), and its calls share the stream and the workspaces of
 * the 1-D density objects, serialised by the caller in the same way.  Every evaluation returns the raw, untruncated sum
 *   S(a, b) = sum_j exp(-((x_j - a) q_x)^2 - ((y_j - b) q_y)^2)
 * (KDE2D.density, kde.py:272-275, without `norm`, which the caller applies); q_x and q_y are finite and positive.
 * Repeated calls are bit-identical, and a point's value does not depend on the other points of a call.  Every call
 * names the handle: a pointer that is not a live object of it (one already destroyed, say) is GPMI_ERR_ARG. */
typedef struct gpmi_kde2d gpmi_kde2d;
int gpmi_kde2d_create(gpmi_ctx* ctx, int64_t n, const double* x_host, const double* y_host, gpmi_kde2d** out);
int gpmi_kde2d_destroy(gpmi_ctx* ctx, gpmi_kde2d* kde);
/* S at the m >= 0 finite points (a_host[i], b_host[i]) (m = 0 returns at once) */
int gpmi_kde2d_eval(gpmi_ctx* ctx, gpmi_kde2d* kde, int64_t m, const double* a_host, const double* b_host, double q_x,
                    double q_y, double* sum_host);
/* S at every sample, in the order the samples were given (sum_host[n]).  Tiles of samples whose every term is below
 * e^-80 are skipped (S_i >= 1 here: what is left out is below 4e-26).  tiles_host, if not NULL, receives the number of
 * tile pairs computed and the nominal number ({done, total}; a tile is 256 samples). */
int gpmi_kde2d_self(gpmi_ctx* ctx, gpmi_kde2d* kde, double q_x, double q_y, double* sum_host, int64_t* tiles_host);
/* S on the grid of an x axis (g_x finite values) and a y axis (g_y values), sum_host[b * g_x + a] = S(x_axis[a],
 * y_axis[b]), as the product of the two factor matrices exp(-((x_j - a) q_x)^2), exp(-((y_j - b) q_y)^2) (fp64 MFMA) */
int gpmi_kde2d_grid(gpmi_ctx* ctx, gpmi_kde2d* kde, int64_t g_x, const double* x_axis_host, int64_t g_y,
                    const double* y_axis_host, double q_x, double q_y, double* sum_host);

/* ---- UnimodalPdf, inference/pdf/unimodal.py ------------------------------------------
 * A unimodal object holds a sample on the device, in the order given (the reduced first stage of the fit reads
 * sample[::skip]); the handle owns it (gpmi_destroy releases the objects still alive), and its calls share the stream
 * and the workspaces of the density objects above, serialised by the caller in the same way.  Every call names the
 * handle: a pointer that is not a live object of it is GPMI_ERR_ARG. */
typedef struct gpmi_unimodal gpmi_unimodal;
int gpmi_unimodal_create(gpmi_ctx* ctx, int64_t n, const double* sample_host, gpmi_unimodal** out);
int gpmi_unimodal_destroy(gpmi_ctx* ctx, gpmi_unimodal* pdf);
/* Replaces the sum of UnimodalPdf.posterior (unimodal.py:132-134, the model of :144-151) for n_theta >= 1 parameter
 * vectors theta = (x0, s0, ln v, f, k, q) at once, over every stride-th sample (stride >= 1):
 *   out_host[t] = sum over i = 0, stride, 2 stride, ... < n of -(1 + v) / 2 * log(1 + |z_i|^q / v),   v = exp(ln v),
 *   z_i = z0_i exp(-f tanh(z0_i / k)),   z0_i = (sample[i] - x0) / s0
 * The caller subtracts n_fit log(norm(theta)).  theta is not checked: non-finite or out-of-range values give what IEEE
 * arithmetic gives (NaN in, NaN out), as the reference's NumPy does.  The sum is reduced in a fixed order that depends
 * on n and stride alone: one theta alone and the same theta inside a batch give the same bits, as do repeated calls. */
int gpmi_unimodal_logpdf_sums(gpmi_ctx* ctx, gpmi_unimodal* pdf, int64_t stride, int n_theta,
                              const double* theta_host, double* out_host);

/* ---- highest-density intervals of the columns of a sample (inference/pdf/hdi.py:6-105) ----
 * Replaces sample_hdi's sort, window widths and argmin (hdi.py:94-104) for m columns of n rows and n_frac window lengths
 * at once.  For column c sorted ascending into s and window length L = L_host[f]:
 *   L <  n : i* = the lowest i in [0, n - L) that attains min (s[i + L] - s[i]);
 *            hdi_host[(2 f) m + c] = s[i*], hdi_host[(2 f + 1) m + c] = s[i* + L]      (L = 0 gives (s[0], s[0]))
 *   L >= n : (s[0], s[n - 1])
 * The caller computes L = int(fraction * n) itself.  A finite column gives exactly the reference's doubles (comparisons
 * and one fp64 subtraction), whatever the other columns, fractions, layout or workspace cap of the call, and repeated
 * calls are bit-identical.  flag_host[c] is 1 if column c holds a NaN or an infinity, else 0: the numbers of a flagged
 * column are unspecified (the kernels stay in bounds and terminate on it), and the caller recomputes it.
 * sample_host is read in place, element (r, c) at sample_host[r * row_stride + c * col_stride] (strides in elements),
 * in one of two dense layouts: (ld, 1) with ld >= m (C order), transposed on the device, or (1, ld) with ld >= n
 * (column-contiguous); m = 1 with row_stride = 1 is one contiguous run.  Anything else is GPMI_ERR_ARG, as are n < 2,
 * m < 1, n_frac < 1 or > 65535 and a negative L.
 * Device memory: the columns are walked in blocks of at most 65535 that fit ws_bytes (0: 4 GiB); the workspace belongs to
 * the handle and is kept for later calls.  A column costs 8 n bytes, twice that in C order and 8 n more for n > 8192,
 * plus 16 n_frac (1 + ceil(n / 4096)) + 4; about 2 KiB + 8 n_frac are fixed.  If one column does not fit the cap the
 * call is GPMI_ERR_ARG and the error text says so.  n <= 2^30 (which needs ws_bytes of 32 GiB or more).
 * Synchronous on the stream of the density entry points above, and serialised by the caller in the same way. */
int gpmi_hdi_columns(gpmi_ctx* ctx, int64_t n, int64_t m, int64_t row_stride, int64_t col_stride,
                     const double* sample_host, int n_frac, const int64_t* L_host, int64_t ws_bytes,
                     double* hdi_host /* n_frac x 2 x m */, int32_t* flag_host /* m */);

/* ---- autocorrelation sums of the columns of a sample (inference/mcmc/utilities.py:83-95) ----
 * Replaces the FFT autocorrelation, the cut at the first negative lag and the sum of effective_sample_size for m columns
 * of n rows at once.  For column c, with y = x - mean(x) in fp64:
 *   f[k] = sum over t < n of y[t] y[(t + k) mod n]        (the circular autocorrelation of length n, for every n)
 *   cut_host[c] = the lowest k in [1, n / 2) with f[k] < 0,   f0_host[c] = f[0],   sum_host[c] = sum over k < cut of f[k]
 * and the caller finishes the effective sample size as int(n / (sum / f0)).  For even n this is what the reference's
 * irfft(|rfft(y)|^2) holds, to rounding; for odd n the reference's irfft returns n - 1 points, which is not an
 * autocorrelation of the sample, and this entry point does not reproduce it.
 * flag_host[c] is 0 for an answered column, 1 if the column holds a NaN or an infinity, 2 if no such k exists (which
 * includes n < 4 and f[0] == 0, a constant column): the numbers of a flagged column are unspecified (the kernels stay in
 * bounds and terminate on it).
 * Every sum is reduced in an order that depends on n alone, without atomics: a column alone and the same column inside a
 * batch give the same bits, whatever the layout or the workspace cap, and repeated calls are bit-identical.  The mean is
 * a fixed-order fp64 sum over n: integer-valued data has an exact mean, so a constant column gives y = 0.
 * The lags are summed in rounds, one block of lags per round (gpmi_acf_lag_blocks), for the columns that have not met
 * a negative lag yet: the work of a column is n (cut rounded up to the end of its block) products.
 * Layouts and strides are those of gpmi_hdi_columns: (ld, 1) with ld >= m (C order), transposed on the device, or
 * (1, ld) with ld >= n; m = 1 with row_stride = 1 is one contiguous run.  Anything else is GPMI_ERR_ARG, as are n < 2
 * and m < 1.
 * Device memory: the columns are walked in blocks of at most 65535 that fit ws_bytes (0: 4 GiB); the workspace belongs to
 * the handle and is kept for later calls.  A column costs 8 (n + n / 2) bytes, 8 n more in C order, 8 ceil(n / 2048) B
 * for the partial sums (B the largest block of gpmi_acf_lag_blocks(n): 256 .. 2048 lags) and 36; 2304 bytes are fixed.
 * If one column does not fit the cap the call is GPMI_ERR_ARG and the error text says so.  n <= 2^30.
 * Synchronous on the stream of the density entry points above, and serialised by the caller in the same way. */
int gpmi_acf_columns(gpmi_ctx* ctx, int64_t n, int64_t m, int64_t row_stride, int64_t col_stride,
                     const double* sample_host, int64_t ws_bytes, double* f0_host /* m */, double* sum_host /* m */,
                     int64_t* cut_host /* m */, int32_t* flag_host /* m */);
/* Host-only (no device call): the first lags of the blocks that gpmi_acf_columns walks for n >= 2 rows, ascending from 0
 * and below n / 2 (256, 256, 512, 1024 and then 2048 lags each).  *count receives their number; starts_host, if not
 * NULL, the first `cap` of them (fewer than *count: GPMI_ERR_ARG). */
int gpmi_acf_lag_blocks(int64_t n, int64_t cap, int64_t* starts_host, int64_t* count);

/* ---- covariance matrix of the columns of a sample (inference/mcmc/pca.py:98-108: numpy.cov) ----
 * What numpy.cov(sample.T) computes for m columns of n rows, in two passes on the device:
 *   mean_host[c] = fl(sum over t of x[t][c] / n),   y = x - mean in fp64,   S = y^T y on the fp64 matrix cores,
 *   cov_host[i * m + j] = S[i][j] * fl(1.0 / (n - 1))           (a product with the rounded reciprocal, as NumPy's)
 * The rows are cut into chunks of GPMI_COV_CHUNK_ROWS.  A column's sum is reduced in a fixed order (inside a chunk four
 * interleaved partial sums over ascending rows, added in order; then the chunks in ascending order), and S[i][j] is one
 * chain of 16 x 16 x 4 matrix-core accumulations over the rows of a chunk, from its first row on, and one chain of
 * additions over the chunks in ascending order, without atomics.  Both orders are fixed by n alone, so
 *   - cov[i][j] depends on columns i and j and on n alone: it has the same bits when the two columns are passed alone,
 *     inside any batch, at any column position, in either layout, under any ws_bytes and on repeated calls;
 *   - cov is symmetric bit for bit (the upper triangle is computed and mirrored);
 *   - integer-valued data whose column sums are multiples of n (and stay below 2^53) has an exact mean, and with
 *     |S| < 2^53 the whole result is NumPy's bit for bit.
 * flag_host[c] is 1 if column c holds a NaN or an infinity, else 0: the rows and columns of cov that involve a flagged
 * column are unspecified (the kernels stay in bounds and terminate on it); the others are not affected.
 * Layouts and strides are those of gpmi_hdi_columns: (ld, 1) with ld >= m (C order) or (1, ld) with ld >= n, both read
 * by the kernels as they lie; m = 1 with row_stride = 1 is one contiguous run.  2 <= n <= 2^30 and 1 <= m <= 512;
 * anything else is GPMI_ERR_ARG with an error text, and the handle stays usable.
 * Device memory: the sample (8 n m bytes), 12 ceil(n / GPMI_COV_CHUNK_ROWS) mp for the chunk sums (mp = m rounded up to
 * 64) and a few tiles belong to the handle's workspace and are kept for later calls.  ws_bytes (0: 1 GiB) caps the
 * partial tiles alone: a chunk costs 32768 T (T + 1) / 2 bytes (T = mp / 64), and the chunks are walked in groups that
 * fit the cap - the bits do not change.  If one chunk does not fit the cap the call is GPMI_ERR_ARG and the text says so.
 * Synchronous on the stream of the density entry points above, and serialised by the caller in the same way. */
#define GPMI_COV_CHUNK_ROWS 2048
int gpmi_cov_columns(gpmi_ctx* ctx, int64_t n, int64_t m, int64_t row_stride, int64_t col_stride,
                     const double* sample_host, int64_t ws_bytes, double* mean_host /* m */,
                     double* cov_host /* m x m, row-major */, int32_t* flag_host /* m */);

/* ---- joint draws from a Gaussian posterior (an addition: the reference's demos call numpy.random.multivariate_normal on
 * the output of build_posterior, regression.py:421-449) ----
 * D = mu + Z L^T with L L^T = Sigma + eps I, eps = jitter_rel * max_j Sigma[j][j], all on the device: neither Sigma nor Z
 * visits the host.  Z is the caller's (z_host) or the library's own counter-based stream of standard normals:
 *   element (s, j) of the stream of `seed` depends on (seed, s, j) alone.  With p = j / 2, one Philox4x32-10 block
 *   (Random123: multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; ten rounds) with the key
 *   (seed & 0xffffffff, seed >> 32) of the seed's 64-bit pattern and the counter (p, s & 0xffffffff, s >> 32, 0) gives
 *   the words r0..r3,  u1 = ((r0 >> 5) 2^26 + (r1 >> 6) + 1) 2^-53 in (0, 1],  u2 = ((r2 >> 5) 2^26 + (r3 >> 6)) 2^-53 in
 *   [0, 1), and with r = sqrt(-2 ln u1), a = fl(2 pi) u2:  Z[s][2 p] = r cos a,  Z[s][2 p + 1] = r sin a (Box-Muller; for
 *   odd m the last sine is dropped).  Row s of a call is draw first_draw + s of the stream.
 * Invariants: the fitted state of gpmi_fit is not touched; row s of the result depends on (model, points, jitter_rel,
 * seed or z row, first_draw + s) alone - not on n_draws, not on the panels the draws are processed in (at most
 * GPMI_DRAWS_PANEL rows at a time, so n_draws is unbounded while the workspace is not), not on where first_draw starts -
 * and repeated calls are bit-identical: the product runs on the tile kernels whose order of summation does not depend on
 * the number of row tiles, and nothing is reduced with atomics.
 * Numerical failure is not an error status: if the largest diagonal entry of Sigma is not finite and positive, info = 1; if
 * the factorisation fails, info = k > 0, the order of the leading minor (within the first m rows) that is not positive
 * definite.  In both cases draws_host is left untouched, the call returns GPMI_OK and the handle stays usable.
 * GPMI_ERR_ARG: m < 1 or m > GPMI_DRAWS_MAX_M, n_draws < 1, first_draw < 0, jitter_rel negative or not finite, a NULL
 * pts_host / mean_host / cov_host / draws_host.
 * Device memory, owned by the call: Sigma (mp (mp + 32) doubles, mp = m rounded up to 128; factorised in place), the
 * inverses of its diagonal blocks (128 mp), one panel of Z and one of D (rows (mp + 32) each, rows = min(n_draws rounded
 * up to 128, GPMI_DRAWS_PANEL)); gpmi_posterior_draws also uses the handle's query workspace, as gpmi_posterior does. */
#define GPMI_DRAWS_MAX_M 16384
#define GPMI_DRAWS_PANEL 4096
/* S joint draws of the latent function at m points from the model of gpmi_fit (one stationary kernel or a sum,
 * any noise model gpmi_posterior serves):  D[s][j] = mu[j] + sum_{k<=j} L[j][k] Z[s][k],  L L^T = Sigma + eps I,
 * Sigma = K_qq - Q^T Q as gpmi_posterior, eps = jitter_rel * max_j Sigma[j][j].  (No data noise in K_qq; the host adds
 * the mean function at the points.)  Without a fit, or after gpmi_fit_dense / gpmi_fit_mix: GPMI_ERR_ARG - such a caller
 * passes its own mean and covariance to gpmi_mvn_draws. */
int gpmi_posterior_draws(gpmi_ctx*, const double* pts_host, int64_t m, double jitter_rel, int64_t n_draws,
                         const double* z_host /* n_draws x m, or NULL: generated */, int64_t seed, int64_t first_draw,
                         double* mu_host /* m, may be NULL */, double* draws_host /* n_draws x m */,
                         double* eps_host /* 1, may be NULL */, int* info);
/* the same tail for a caller's mean (m) and covariance (m x m row-major, lower triangle read); needs no data set */
int gpmi_mvn_draws(gpmi_ctx*, int64_t m, const double* mean_host, const double* cov_host, double jitter_rel,
                   int64_t n_draws, const double* z_host, int64_t seed, int64_t first_draw,
                   double* draws_host, double* eps_host, int* info);
/* host-only, no device call: rows first_draw .. first_draw + n_draws - 1 of the generator's stream (n_draws x m), from the
 * same integer code with the host's libm: within a few units in the last place of the device's */
int gpmi_draws_normals(int64_t seed, int64_t first_draw, int64_t n_draws, int64_t m, double* z_host);

/* ---- large data: the variational inducing-point approximation (Titsias 2009; an addition, the reference has none) ----
 * N data points x (N x d) are summarised by m << N fixed inducing inputs Z (m x d): O(N m^2) time, O(N d + m^2) memory.
 * With r = y - mu(x) (the caller's residual), sigma_i^2 = noise_var_i + white_var, W = diag(1 / sigma_i^2), k one
 * stationary kernel of prior variance a^2 and eps = jitter_rel a^2:
 *   K_mm + eps I = L L^T        G = K_mn W K_nm        H = L^-1 G L^-T (symmetrised)        B = I + H = L_B L_B^T
 *   c = L_B^-1 L^-1 K_mn W r
 *   F = -1/2 [N ln 2 pi + sum ln sigma_i^2 + 2 sum ln diag(L_B) + r^T W r - c^T c] - 1/2 [a^2 sum_i 1 / sigma_i^2 - tr H]
 *   mean(q) = u^T c,   var(q) = a^2 - |v|^2 + |u|^2,   v = L^-1 k_m(q),   u = L_B^-1 v       (the latent f: no noise added)
 * F is a lower bound of the log marginal likelihood (with its 2 pi constant) and equals it for Z = x, eps = 0.  Only B is
 * ever factorised besides K_mm + eps I - never the N x N matrix, never K_mm^-1 times a data-sized array.
 * K_mn is never held whole: x is walked in panels of `panel_rows` rows (0: the default, 8192; rounded up to a multiple of
 * 128), one panel (m_pad x panel doubles) at a time, twice for a gradient.  F, the gradient and alpha may depend on
 * panel_rows in their last digits (the grouping of the sums over the data changes); for given arguments every result is
 * bit-reproducible: fixed-order reductions, no atomics.
 * The gradient (n_theta + 1 values: the kernel's parameters in theta's order, then dF / d ln s with white_var = s^2,
 * which is 0 for white_var = 0) includes d eps / d ln a = 2 eps.  alpha = W (r - K_nm gamma), gamma = (K_mm + eps I + G)^-1
 * K_mn W r (N values): the mean function's gradient is (d mu / d theta)^T alpha on the host.
 * info > 0 is not an error status: K_mm + eps I (info = the order of the leading minor that is not positive definite,
 * 1..m) or B (m + that order) could not be factorised; F, grad and alpha are then untouched, the call returns GPMI_OK and
 * the object stays usable.  GPMI_ERR_ARG (text via gpmi_last_error, object still usable): a NULL pointer that is not
 * optional, a kernel other than GPMI_KERNEL_SE / _RQ / _M32 / _M52, an n_theta that does not match kernel and d, white_var
 * or jitter_rel negative or not finite, panel_rows negative, noise_var_i + white_var not positive for some i (checked on
 * the device), gpmi_sgp_bound / _fit before gpmi_sgp_set_targets, gpmi_sgp_predict before a successful gpmi_sgp_fit.
 * Limits: 1 <= m <= GPMI_SGP_MAX_M, 2 <= n <= 2^30, d <= 64; m <= n is not required.
 * gpmi_sgp_bound does not touch the state gpmi_sgp_fit left: predictions before and after it are bit-identical.
 * Device memory of an object: x, Z, r, the noise variances and two more vectors of n doubles (1 / sigma_i^2, alpha); eleven
 * matrices of m_pad (m_pad + 32) doubles (m_pad = m rounded up to 128; nine of work, two of the fit); three panels of
 * max(m_pad, panel) x (max(m_pad, panel) + 32) doubles at most, allocated at the first call that needs them; behind the
 * first gpmi_sgp_bound_zgrad m_pad x d doubles (dF/dZ) and its partial sums, m_pad x d x max(panel, m_pad) / 1024 doubles
 * (for m_pad x panel < 2^19 up to eight times that, and never more than 32 MiB then).
 * Objects belong to their handle (calls on one handle are serialised); gpmi_destroy releases those still alive. */
#define GPMI_SGP_MAX_M 4096
#define GPMI_SGP_PANEL 8192
typedef struct gpmi_sgp gpmi_sgp;
int gpmi_sgp_create(gpmi_ctx* ctx, int64_t n, int64_t d, const double* x_host /* n x d */, int64_t m,
                    const double* z_host /* m x d */, gpmi_sgp** out);
/* release an object (NULL, or not a live object of its handle: GPMI_ERR_ARG); not after gpmi_destroy of the handle */
int gpmi_sgp_destroy(gpmi_sgp* sgp);
/* the residual r = y - mu(x) and the data variances y_err^2 (NULL: all zero), n values each; they stay on the device */
int gpmi_sgp_set_targets(gpmi_sgp* sgp, const double* r_host, const double* noise_var_host);
int gpmi_sgp_bound(gpmi_sgp* sgp, int kernel, const double* theta, int n_theta, double white_var, double jitter_rel,
                   int64_t panel_rows, double* F, double* grad /* n_theta + 1, may be NULL */,
                   double* alpha_host /* n, may be NULL */, int* info);
/* gpmi_sgp_bound plus dF/dZ: F, grad (n_theta + 1, may be NULL) and alpha exactly as gpmi_sgp_bound returns them - the same
 * bits - and grad_z (m x d, row i = dF/dz_i, required).  With M1 = gamma alpha^T + T K_mn W, M2 = gamma gamma^T + K_mm^-1 G
 * K_mm^-1 - T (T = K_mm^-1 - (K_mm + G)^-1, with eps in K_mm), s_ij = 1/2 sum_k D_k^2 / l_k^2 and g the profile of
 * dK / d ln l_k = a^2 g(s) D_k^2 / l_k^2:
 *   dF/dz_ik = -1 / l_k^2 [sum_j M1_ij a^2 g(s(z_i, x_j)) (z_ik - x_jk) - sum_j M2_ij a^2 g(s(z_i, z_j)) (z_ik - z_jk)]
 * (eps does not depend on Z; nothing is divided by a distance: coincident points contribute exact zeros).  The contraction
 * runs behind the theta-gradient's on the same panels - no panel and no product is rebuilt - with sums whose order is
 * fixed by (n, m, d, panel_rows): bit-reproducible, no atomics.  info != 0 leaves the outputs undefined, as there. */
int gpmi_sgp_bound_zgrad(gpmi_sgp* sgp, int kernel, const double* theta, int n_theta, double white_var, double jitter_rel,
                         int64_t panel_rows, double* F, double* grad /* n_theta + 1, may be NULL */,
                         double* grad_z /* m x d */, double* alpha_host /* n, may be NULL */, int* info);
/* replace the inducing inputs (same m, same d).  Non-finite values: GPMI_ERR_ARG, the old Z stays.  A fit kept by
 * gpmi_sgp_fit is dropped: gpmi_sgp_predict before the next successful fit is GPMI_ERR_ARG, the object stays usable. */
int gpmi_sgp_set_inducing(gpmi_sgp* sgp, const double* z_host /* m x d */);
/* the bound, and L^-1, L_B^-1, c and the kernel's parameters kept for gpmi_sgp_predict (kept only if info == 0; a failed
 * fit leaves the previous one in place) */
int gpmi_sgp_fit(gpmi_sgp* sgp, int kernel, const double* theta, int n_theta, double white_var, double jitter_rel,
                 int64_t panel_rows, double* F, int* info);
/* mean and variance of the latent function at mq points (panels of 1024 points); var_host may be NULL */
int gpmi_sgp_predict(gpmi_sgp* sgp, const double* pts_host /* mq x d */, int64_t mq, double* mean_host,
                     double* var_host);
/* ---- the fitted sparse model beyond mean and variance: joint posterior, joint draws, derivatives by the query point ----
 * All three need a successful gpmi_sgp_fit (otherwise, and after gpmi_sgp_set_inducing without a new fit, GPMI_ERR_ARG and
 * the object stays usable), leave the fit and every later result bit-identical, return GPMI_OK for mq == 0 without doing
 * anything, and answer a NULL pointer that is not optional with GPMI_ERR_ARG.  They cost O(mq m^2) whatever N is.
 *
 * Joint posterior of the latent function (no data noise, as gpmi_posterior) at mq <= GPMI_DRAWS_MAX_M points Q.  With the
 * rows V = [v(q_1) .. v(q_mq)]^T, U likewise (mq x m), v = L^-1 k_m(q), u = L_B^-1 v:
 *   mean = U c,   cov = K_qq - V V^T + U U^T     (its diagonal is gpmi_sgp_predict's variance up to rounding)
 * on the kernels of the fit: the cross builds, the two products with the kept inverses for all mq rows at once, the two
 * Gram updates on the lower tiles (the product only subtracts: the sign of the matrix is turned in between), the mirror
 * into the upper triangle - cov_host is symmetric bit for bit.  cov_host == NULL: the mean alone.
 * Device memory, owned by the call and released at return: the points, V and U (mq_pad (m_pad + 32) doubles each, mq_pad =
 * mq rounded up to 128) and, with cov_host, Sigma (mq_pad (mq_pad + 32) doubles). */
int gpmi_sgp_posterior(gpmi_sgp* sgp, const double* pts_host /* mq x d */, int64_t mq, double* mean_host /* mq */,
                       double* cov_host /* mq x mq, symmetric, may be NULL */);
/* n_draws joint draws of the latent function at mq <= GPMI_DRAWS_MAX_M points: mean and Sigma as gpmi_sgp_posterior forms
 * them stay on the device and go to the tail gpmi_posterior_draws and gpmi_mvn_draws share - D = mu + Z L^T, L L^T = Sigma +
 * eps I, eps = jitter_rel * max_j Sigma[j][j], Z the caller's or the generator's stream.  Arguments, the generator, info
 * (> 0: not an error status, draws_host untouched, GPMI_OK), eps_host and the invariants are gpmi_posterior_draws's; Sigma
 * is numerically singular from a hundred points on, so jitter_rel = 0 rarely factorises.  The sparse work runs on the sparse
 * stream and is waited for before the tail starts on the handle's first lane (created, streams and events alone, if the
 * handle never held an exact model).  Device memory of the call: gpmi_sgp_posterior's plus the tail's (gpmi_posterior_draws),
 * all released at return. */
int gpmi_sgp_posterior_draws(gpmi_sgp* sgp, const double* pts_host /* mq x d */, int64_t mq, double jitter_rel,
                             int64_t n_draws, const double* z_host /* n_draws x mq, or NULL: generated */, int64_t seed,
                             int64_t first_draw, double* mean_host /* mq, may be NULL */,
                             double* draws_host /* n_draws x mq */, double* eps_host /* 1, may be NULL */, int* info);
/* d mean / d q and d var / d q at mq points (any mq: panels of 1024 points, as gpmi_sgp_predict), for all four kernels.
 * With k(q, z) = a^2 C(s), s = 1/2 sum_k (q_k - z_k)^2 / l_k^2, g = -dC/ds (the profile of dK / d ln l_k),
 *   gamma = L^-T L_B^-T c (kept by the fit: mean(q) = k_m(q)^T gamma),
 *   t(q) = L^-T (L_B^-T u(q) - v(q))   (var(q) = a^2 + k_m(q)^T t(q); formed from v and u per point, as the variance is),
 *   dmean[j][k] = -1 / l_k^2 sum_a gamma_a  a^2 g(s(q_j, z_a)) (q_jk - z_ak),
 *   dvar [j][k] = -2 / l_k^2 sum_a t_a(q_j) a^2 g(s(q_j, z_a)) (q_jk - z_ak).
 * Nothing is divided by a distance: a query point that is an inducing input gets an exact zero from that input.
 * Accuracy: dmean contracts k'(q) with gamma, whose entries grow and cancel as K_mm + eps I loses condition (the mean
 * itself, u^T c, does not): its error scales with cond(K_mm + eps I) - measured 1e-6 relative at cond 1e6 (m = 512 random
 * rows of 1e5 points, profiles/r19_sparse_post.txt), 1e-12 at the well-conditioned shapes of the tests; dvar, formed from
 * v and u, kept eight digits there.  Spread inducing inputs, or a larger jitter_rel, where the gradient matters.  One fused
 * kernel forms the profile once for both sums; dvar_host == NULL skips the four products behind t and the second sum, and
 * dmean_host has the same bits either way.  Row j of both results depends on (fit, q_j) alone: the same bits whether q_j is
 * evaluated alone or anywhere inside a larger call, and on repeated calls - the sums over the inducing inputs have an order
 * fixed by m alone (no atomics), the products run on tile shapes that do not depend on mq.
 * Device memory, kept by the object from the first call on: m_pad / 128 + 1 times 2 x 1024 x d doubles (the partial sums per
 * run of 128 inducing inputs and the panel's results), besides the three query panels of gpmi_sgp_predict. */
int gpmi_sgp_spatial_derivatives(gpmi_sgp* sgp, const double* pts_host /* mq x d */, int64_t mq,
                                 double* dmean_host /* mq x d */, double* dvar_host /* mq x d, may be NULL */);
/* Host-only (no device call): the size-dependent schedule of gpmi_sgp_bound / _bound_zgrad / _fit for n data points, m
 * inducing points and the caller's panel_rows, from the functions the launches themselves call.  out = {P, the rows of x per
 * panel; m_pad; the 64-row tiles one workgroup of the dF/dZ contraction sums over a data panel (2, 4, 8 or 16); the same for
 * its K_mm term; the workgroups of the pass that forms 1 / sigma_i^2 (at most 1024: beyond 262144 points a workgroup strides);
 * the number of panels, ceil(n / P)}.  GPMI_ERR_ARG on the ranges of gpmi_sgp_create and gpmi_sgp_bound: n outside 2 .. 2^30,
 * m outside 1 .. GPMI_SGP_MAX_M, panel_rows outside 0 .. 32768, out NULL.  The tests use it to prove which branch they ran. */
int gpmi_sgp_schedule(int64_t n, int64_t m, int64_t panel_rows, int64_t out[6]);

/* ---- lockstep batches of the bound: T hyper-parameter vectors on one object, x, Z and the noise data shared ----
 * gpmi_sgp_bound_batch evaluates F - and, where grad is not NULL, dF/dtheta in gpmi_sgp_bound's layout - for the T rows of
 * thetas_host with the WhiteNoise variance white_var_host[t] each.  Every launch of gpmi_sgp_bound's two passes carries a
 * chunk of problems side by side, and the host is waited for once per chunk, not per panel or factorisation.
 * Residuals: gpmi_sgp_set_observations puts y itself (n doubles more) and the data variances on the device (the variances
 * are the object's one copy, the one gpmi_sgp_set_targets writes); row t then works on r_t = y - mu_const_host[t], one
 * subtraction per point on the device (the bits of the host's y - c), or on r_t = y - mus_host[t] (T x n: any mean
 * function).  Exactly one of the two is given.  Nothing of r_t comes from gpmi_sgp_set_targets: a row does not depend on
 * the object's history, and the batch call leaves the residual of gpmi_sgp_set_targets, the kept fit and every later
 * single evaluation bit-identical.
 * Results per row: F[t]; grad (n_theta + 1 values); sum_alpha[t] = sum_i alpha_ti, reduced on the device in a fixed order
 * (the gradient by a constant mean); alpha_host (n values, for other mean functions); info[t] in gpmi_sgp_bound's
 * numbering.  Each may be NULL but F and info.  A row with info[t] > 0 is not an error: its other results are
 * unspecified, it writes nowhere but into its own slices and changes no other row.
 * Bits: every sum has an order fixed by (n, m, d, panel_rows) alone, nothing uses atomics, no product takes a tile shape
 * that depends on the number of problems in its launch: a row's F, gradient, sum_alpha and alpha are the same bits alone,
 * at any position of any batch, under any max_chunk and on a repeated call, and F is the same with and without the
 * gradient.  Equality with gpmi_sgp_bound's bits is not promised (its products may take other tile shapes).
 * GPMI_ERR_ARG, before anything is touched: T < 0 (T = 0 returns GPMI_OK at once), a call before
 * gpmi_sgp_set_observations, both or neither of mu_const_host / mus_host, the argument errors of gpmi_sgp_bound for any
 * row - among them noise_var_i + white_var[t] not positive and finite, decided on the host from the range of the
 * variances -, max_chunk < 0.
 * Memory: the workspace belongs to the object, grows on demand, is kept between calls and released with the object.
 * Doubles per problem, with P the rows of a panel, ld = m_pad + 32:
 *   9 m_pad ld + 256 m_pad + (4 m_pad + 3 P) + 128 + 4096 + 3 max(m_pad (P + 32), P ld) + 2 n + 2,
 *   and where a gradient, sum_alpha or alpha is asked for  n + max(P, m_pad) m_pad (d + 2) / 4096  more,
 * plus the problem's parameters (about 550 bytes).  chunk = min(T, 1024, max_chunk if > 0, budget / bytes per problem), at
 * least 1; the budget is GPMI_BATCH_GIB GiB (1 .. 200, by default and otherwise 24), the cap of the other lockstep batches.
 * Chunks run one after another.
 * gpmi_sgp_batch_schedule (host only, no device call) returns what a call with these arguments does, from the function the
 * call itself uses: out = {chunk, number of chunks, bytes per problem, P, panels, m_pad}; want_grad: any of grad,
 * sum_alpha, alpha_host; budget_bytes = 0: the library's.  GPMI_ERR_ARG on the ranges of gpmi_sgp_schedule, d outside
 * 1 .. 64, T, max_chunk or budget_bytes negative, out NULL. */
int gpmi_sgp_set_observations(gpmi_sgp* sgp, const double* y_host /* n */, const double* noise_var_host /* n, or NULL: zero */);
int gpmi_sgp_bound_batch(gpmi_sgp* sgp, int kernel, int64_t T, const double* thetas_host /* T x n_theta */, int n_theta,
                         const double* white_var_host /* T */, const double* mu_const_host /* T, or NULL */,
                         const double* mus_host /* T x n, or NULL */, double jitter_rel, int64_t panel_rows,
                         int64_t max_chunk /* 0: automatic */, double* F /* T */,
                         double* grad /* T x (n_theta + 1), or NULL */, double* sum_alpha /* T, or NULL */,
                         double* alpha_host /* T x n, or NULL */, int* info /* T */);
int gpmi_sgp_batch_schedule(int64_t n, int64_t m, int64_t d, int64_t panel_rows, int64_t T, int want_grad,
                            int64_t max_chunk, int64_t budget_bytes, int64_t out[6]);

/* Greedy conditional-variance selection of inducing points among the rows of x: the pivoted partial Cholesky factorisation
 * of K_nn (the greedy MAP of a k-DPP; Burt, Rasmussen and van der Wilk, JMLR 2020).  It needs no gpmi_sgp object and no
 * gpmi_set_data.  The work is done in unit prior variance, C = K / a^2: theta has the layout of gpmi_sgp_bound, theta[0] =
 * ln a is read and not used.  weight_host: w_i >= 0 (NULL: all 1; for the bound of gpmi_sgp_bound, 1 / sigma_i^2).
 *   State: d_i = 1;  V, count x n, row t contiguous in i;  tr_0 = sum_i w_i.
 *   Step t = 0, 1, ...:
 *   1. eligible are the i with d_i > floor_rel and w_i > 0.  Stop - count = t - if none is left, if t = m_max or if
 *      tr_t <= trace_tol tr_0.
 *   2. the pivot p = argmax over the eligible of w_i d_i, the lowest index among equal scores (numpy.argmax; step 0 without
 *      weights is a tie of ones: row 0).  pivot_var[t] = d_p.
 *   3. c_i = C(x_i, x_p) - sum_{l<t} V_li V_lp in ascending l,  V_ti = c_i / sqrt(d_p).  C(x_i, x_p) has the bits of the
 *      covariance builders (s = sum_k 1/2 dx_k^2 / l_k^2 by one fma per dimension in ascending k, then the kernel's profile),
 *      so V_ti depends on (x_i, the pivots, theta) alone: not on n, not on the place of row i.
 *   4. d_i <- max(d_i - V_ti^2, 0),  d_p <- 0,  tr_{t+1} = sum_i w_i d_i: a sum of fixed order, no atomics.
 * Results: count; index_host[0 .. count): the pivots in the order chosen - the first k are the selection of size k;
 * trace_host[0 .. count]: tr_0 .. tr_count (a^2 tr_k is the trace term a^2 sum w - tr H of the bound at Z = x[first k pivots],
 * jitter 0); pivot_var_host[0 .. count).  Entries beyond count are left untouched.  Repeated calls give the same bits.
 * One launch per step and no host synchronisation between them; a step reads t n doubles of V, a selection moves about
 * 8 n m_max^2 / 2 bytes: it is bound by HBM.
 * Limits: 1 <= n <= 2^30, 1 <= d <= 64, 1 <= m_max <= min(n, GPMI_SGP_MAX_M).
 * GPMI_ERR_ARG (the handle stays usable): a NULL pointer that is not optional; a kernel other than GPMI_KERNEL_SE, _RQ, _M32,
 * _M52; n_theta that does not match the kernel and d; x or theta not finite; weights negative, not finite or without a
 * positive entry; floor_rel or trace_tol negative or not finite.  GPMI_ERR_NOMEM: V could not be allocated.
 * Device memory, allocated for the call and released at return: V, 8 n m_max bytes, x, and two or three vectors of n
 * doubles. */
int gpmi_select_points(gpmi_ctx* ctx, int64_t n, int64_t d, const double* x_host /* n x d */,
                       const double* weight_host /* n, may be NULL */, int kernel, const double* theta, int n_theta,
                       int64_t m_max, double floor_rel, double trace_tol, int64_t* index_host /* m_max */,
                       double* trace_host /* m_max + 1 */, double* pivot_var_host /* m_max, may be NULL */, int64_t* count);
/* Host-only (no device call): out = {the workgroups of a selection step over n points, ceil(n / 256)} - as many block partials
 * as every workgroup reduces at the next launch (beyond 65536 points a thread reads more than one).  n outside 1 .. 2^30 or
 * out NULL: GPMI_ERR_ARG. */
int gpmi_select_schedule(int64_t n, int64_t out[1]);

/* ---- many targets at one set of inputs (MultiTargetGpRegressor) ---------------------
 * T target vectors observed at the handle's x with its data errors and ONE covariance K(theta) (the matrix of gpmi_fit:
 * kernel or sum, + extra_diag I, + the data variances; the y of gpmi_set_data takes no part).  With R = Y - 1 m^T (n x T),
 * K = L L^T, V = L^-1 R and A = K^-1 R:
 *   lml_t = -1/2 |V[:, t]|^2 - sum_i ln L_ii     (no 2 pi term, as gpmi_lml),     lml = sum_t lml_t,
 *   d lml / d theta_j = 1/2 sum_ab (A A^T - T K^-1)_ab (dK / d theta_j)_ab,
 *   mean(q)[t] = k(q)^T A[:, t]  (the caller adds m_t),   var(q) = a^2 - |L^-1 k(q)|^2  (one for all targets).
 * K is built, factorised and - for the gradient - inverted ONCE per call; per target there are the two O(n^2) solves.
 * On the device the targets are rows: T_pad x (n_pad + 32) doubles with T_pad = T rounded up to 128, zeros in the padding;
 * V^T and A^T are one many-right-hand-side forward and one backward solve, the means one product per 2048 query points.
 * Every sum has an order fixed by (n, T): repeated calls return the same bits, and no call uses atomics.
 * gpmi_mt_fit leaves the factor where gpmi_fit leaves it (lane 0) and gpmi_mt_predict's variance is gpmi_predict's, bit
 * for bit.  gpmi_mt_lml, gpmi_mt_lml_grad and gpmi_mt_loo_terms evaluate other hyper-parameters on lane 1: the fit and
 * every later answer of it keep their bits.
 * A matrix that does not factorise is reported through info > 0 (lml and lml_t are then -1e50, the other outputs
 * undefined), not through the status.
 * GPMI_ERR_ARG, with the handle still usable: T outside 1 .. GPMI_MT_MAX_T; any of these calls before
 * gpmi_mt_set_targets - a gpmi_set_data drops the targets with the rest of the data set -; gpmi_mt_alpha, gpmi_mt_predict
 * or gpmi_mt_loo without a successful gpmi_mt_fit as the handle's last fit; the kernel / n_theta errors of gpmi_fit.
 * Device memory, owned by the handle and released with it or at the next gpmi_set_data / gpmi_mt_set_targets, each buffer
 * allocated by the first call that needs it: 8 T_pad (n_pad + 32) bytes for the targets, as much for the fit's A^T and for
 * the evaluations' V^T / A^T; 8 n_pad (T_pad + 32) for the transposed copies; 8 * 2048 (T_pad + 32 + T) for a chunk of
 * means; three short vectors. */
#define GPMI_MT_MAX_T 4096
/* r_host: n x T row-major, the residuals Y - 1 m^T.  Replaces an earlier target matrix of the handle. */
int gpmi_mt_set_targets(gpmi_ctx* ctx, const double* r_host /* n x T */, int64_t T);
/* Fit at theta: L into lane 0 by gpmi_fit's own stages, A^T kept for gpmi_mt_alpha / _predict / _loo. */
int gpmi_mt_fit(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
                double* lml_t_host /* T, or NULL */, double* lml /* or NULL */, int* info);
int gpmi_mt_lml(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
                double* lml_t_host /* T, or NULL */, double* lml /* or NULL; not both */, int* info);
/* grad_host: n_theta + 1 values - d lml / d theta_j as gpmi_lml_grad lays them out, then T times its trace_q,
 * sum_i (sum_t A_it^2 - T (K^-1)_ii): d lml / d extra_diag is half of it.  K^-1 is formed as in gpmi_lml_grad, A A^T / T is
 * subtracted from its lower tiles by one product with k = T_pad, and gpmi_lml_grad's contraction runs once with u = v = 0;
 * the transposed copy A / sqrt(T) (n_pad rows) is tiled through LDS. */
int gpmi_mt_lml_grad(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag, double* lml,
                     double* grad_host /* n_theta + 1 */, int* info);
/* The leave-one-out terms at theta: a2_i = sum_t A_it^2 and (K^-1)_ii.  With var_i = 1 / (K^-1)_ii the leave-one-out
 * log-likelihood of all targets is -1/2 sum_i (var_i a2_i + T ln var_i). */
int gpmi_mt_loo_terms(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double extra_diag,
                      double* a2_host /* n */, double* ikdiag_host /* n */, int* info);
/* A of the fit, n x T row-major: column t is the alpha of the single-target model of target t. */
int gpmi_mt_alpha(gpmi_ctx* ctx, double* alpha_host /* n x T */);
/* mean_host: m x T row-major, k(q)^T A without the offsets m_t; var_host: m values a^2 - |L^-1 k(q)|^2, or NULL. */
int gpmi_mt_predict(gpmi_ctx* ctx, const double* pts_host /* m x d */, int64_t m, double* mean_host /* m x T */,
                    double* var_host /* m, or NULL */);
/* Leave-one-out residuals of the fit: resid_loo[i][t] = A_it / (K^-1)_ii (the prediction is Y_it minus it), and (K^-1)_ii.
 * Uses lane 1's second matrix for L^-T, as gpmi_loo_diag. */
int gpmi_mt_loo(gpmi_ctx* ctx, double* resid_loo_host /* n x T */, double* ikdiag_host /* n */);

/* ---- non-Gaussian likelihoods by Laplace's method (GeneralisedGpRegressor) ----------
 * A latent GP f = m + K a (K: the kernel's covariance of the handle's x with its a^2 1e-12 jitter, no data errors, no
 * extra_diag; m a constant offset) observed through a log-concave likelihood p(y_i | f_i) with per-point data aux_i:
 *   GPMI_GGP_LOGISTIC  robust regression: log p = z - 2 softplus(z) - ln s, z = (y - f) / s, aux = s > 0, y real
 *   GPMI_GGP_POISSON   counts, log link:  log p = y (f + ln e) - e exp(f) - lgamma(y + 1), aux = e > 0, y = 0, 1, 2, ..
 *   GPMI_GGP_BINOMIAL  k of n, logit link: log p = y f - n softplus(f) + ln C(n, y), aux = n >= 1, y = 0 .. n
 * The mode of psi(a) = -1/2 a^T (f - m) + sum_i log p(y_i | f_i) is found by Newton's iteration from a = 0 (GPML Alg. 3.1):
 * with g = d log p / df, W = -d^2 log p / df^2 >= 0, sw = sqrt W a step factorises B = I + sw sw^T o K = L L^T (eigenvalues
 * >= 1), sets b = W (f - m) + g, a+ = b - sw o B^-1 (sw o K b), f+ = m + K a+, halves the step along a+ - a (at most ten
 * times) while psi(a+) < psi(a) - 1e-12 |psi(a)|, and stops when max |f+ - f| <= tol (1 + max |f+|).  B is then factorised
 * once more at the final f, and  log q(y | theta) = psi - sum_i ln L_ii  (GPML eq. 3.32).  Every evaluation starts from
 * a = 0: a value depends on theta alone.  The host reads one small record per step; everything else stays on the device.
 * gpmi_ggp_fit runs on lane 0 and keeps the factor for gpmi_ggp_mode / gpmi_ggp_predict; gpmi_ggp_logq and
 * gpmi_ggp_logq_grad evaluate other hyper-parameters on lane 1: the fit and every later answer of it keep their bits.
 * No call uses atomics and every sum has an order fixed by the padded n: repeated calls return the same bits.
 * info: 0 success; k > 0: B was not positive definite (or not finite) at leading minor k; -1: no convergence within
 * max_iter steps, or psi not finite.  With info != 0 logq is -1e50, the other outputs are undefined, the status is GPMI_OK
 * and (gpmi_ggp_fit) the handle holds no fit.  out_iters: {Newton steps, step halvings}.
 * GPMI_ERR_ARG, before anything is launched and with the handle still usable: a likelihood id other than the three; NULL
 * y / aux; a value of y or aux outside the domain above or not finite; an offset that is not finite; any other call
 * before gpmi_ggp_set_observations (gpmi_set_data drops the observations with the rest of the data set); a kernel other
 * than GPMI_KERNEL_SE / _RQ / _M32 / _M52 and the n_theta errors of gpmi_fit; tol not in (0, 1), max_iter < 1; NULL outputs;
 * gpmi_ggp_mode / gpmi_ggp_predict without a successful gpmi_ggp_fit as the handle's last fit.
 * Device memory, owned by the handle and released with it or at the next gpmi_set_data: per lane one padded matrix for K
 * (8 n_pad (n_pad + 32) bytes) beside the lane's own matrix for B and L - and, for gpmi_ggp_logq_grad, the lane's second
 * matrix -, 18 vectors of n_pad doubles and the block partials; four vectors of n_pad for the observations. */
#define GPMI_GGP_LOGISTIC 0
#define GPMI_GGP_POISSON 1
#define GPMI_GGP_BINOMIAL 2
/* y_host, aux_host: n values each.  Replaces earlier observations of the handle and drops a fit made from them. */
int gpmi_ggp_set_observations(gpmi_ctx* ctx, int likelihood, const double* y_host, const double* aux_host, double offset);
int gpmi_ggp_fit(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double tol, int max_iter, double* logq,
                 int* out_iters /* 2 */, int* info);
int gpmi_ggp_logq(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double tol, int max_iter, double* logq,
                  int* out_iters /* 2 */, int* info);
/* grad_host: d log q / d theta_j, n_theta values, explicit and implicit (through the mode) parts together: with
 * R = sw sw^T o B^-1, s2 = 1/2 (diag K - diag(K R K)) o d3, w = s2 - R K s2 and u = g + 2 w it is
 * 1/2 sum_ab [1/2 (u g^T + g u^T) - R]_ab (dK / d theta_j)_ab - one run of gpmi_lml_grad's contraction. */
int gpmi_ggp_logq_grad(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, double tol, int max_iter,
                       double* logq, double* grad_host /* n_theta */, int* out_iters /* 2 */, int* info);
/* the mode f-hat and g = grad log p(y | f-hat) (= a = K^-1 (f-hat - m) at the mode) of the fit, n values each */
int gpmi_ggp_mode(gpmi_ctx* ctx, double* f_host, double* g_host);
/* latent mean m + k(q)^T g and variance a^2 - |L^-1 (sw o k(q))|^2 at m points (var_host may be NULL) */
int gpmi_ggp_predict(gpmi_ctx* ctx, const double* pts_host /* m x d */, int64_t m, double* mean_host, double* var_host);
/* Y = V K^T for nv = 1 .. 4 vectors (rows of V_host, nv x n; Y_host likewise) with the latent K at theta, built on lane 1:
 * the product kernel of the Newton steps on its own (tests, tools/generalised_bench.py).  reps >= 1 runs of the product;
 * ms (may be NULL): the HIP-event time of all of them. */
int gpmi_ggp_kv(gpmi_ctx* ctx, int kernel, const double* theta_host, int n_theta, const double* V_host, int nv,
                double* Y_host, int reps, float* ms);

/* ---- instrumentation ---------------------------------------------------------------
 * HIP-event timing on the handle's own stream (torch.cuda.Event would not see it). */
int gpmi_timer_start(gpmi_ctx* ctx);
int gpmi_timer_stop(gpmi_ctx* ctx, float* ms);
/* per-kernel-class accounting: when enabled every launch of the class is bracketed by events; the two
 * trailing-update classes (SYRK, SYRK_REST, SYRK_SLICE) are timed by in-kernel stamps instead and cost nothing */
/* Host-only (no device call): the task lists of the flag-ordered factorisation of a tail of `m` tile rows dealt to `nwg`
 * workgroups (csrc/potrf_flow.hip; replaces nothing in the reference - it is the schedule of numpy.linalg.cholesky's
 * replacement, regression.py:241).  out: 8 ints per task {type (0 panel TRSM slab, 1 one-column update of a 64 x 64
 * sub-tile, 2 K = 512 chunk), i, j, k, s, flag increment, owner workgroup, 0}, list after list; out == NULL: only the
 * count.  tests/test_flow_cpu.py replays them with NumPy tile operations. */
int gpmi_flow_task_lists(int m, int nwg, int64_t cap, int32_t* out, int64_t* ntasks);

#define GPMI_PROF_KBUILD 0  /* covariance build            (HBM-write bound) */
#define GPMI_PROF_SYRK 1    /* potrf trailing SYRK/GEMM    (fp64 MFMA bound) */
#define GPMI_PROF_PANEL 2   /* potrf diagonal block + panel TRSM (latency bound) */
#define GPMI_PROF_SOLVE 3   /* single right-hand side triangular sweeps (HBM-read bound) */
#define GPMI_PROF_SYRK_REST 4 /* trailing-update launches that do not run the 128 x 128-tile kernel: the 64 x 64-tile
                                 remainder of a split launch and the launches with fewer than 384 tiles */
#define GPMI_PROF_TRSM 5    /* many right-hand side solves: predict, posterior, L^-T (fp64 MFMA bound) */
#define GPMI_PROF_SYRK_SLICE 6 /* the tiles of a trailing update that run, concurrently with the rest, on the 32 CUs
                                  reserved for the panel chain (same 128 x 128-tile kernel as SYRK) */
#define GPMI_PROF_FLOW 7    /* the flag-ordered tile-task launch of the chain-bound part of a factorisation (potrf_flow.hip):
                               FLOPs of its update tasks over the launch's whole duration - it waits for the panel
                               chain most of the time, so this is the overlap achieved, not a kernel rate */
#define GPMI_PROF_COV 8     /* the kernels of gpmi_cov_columns, from the column sums to the scaled covariance, without the
                               copies to and from the device (HBM-read bound: the sample is read twice) */
/* the four stages of gpmi_posterior_draws / gpmi_mvn_draws (tools/draws_bench.py), each bracketed as a whole */
#define GPMI_PROF_DRAWS_SIGMA 9    /* Sigma: cross-covariances, the many-right-hand-side solve, K_qq - Q^T Q (or the upload) */
#define GPMI_PROF_DRAWS_FACTOR 10  /* max diag, + eps I, the factorisation, the zeroing of the upper triangle */
#define GPMI_PROF_DRAWS_NORMALS 11 /* the normal generator (or the upload of the caller's Z) */
#define GPMI_PROF_DRAWS_PRODUCT 12 /* D = Z L^T + mu */
/* the four stages of gpmi_sgp_bound / gpmi_sgp_fit (tools/sparse_bench.py), each bracketed as a whole */
#define GPMI_PROF_SGP_BUILD 13  /* pass 1: the panels of K_mn (cross build, column scaling, K_mn W r) */
#define GPMI_PROF_SGP_GRAM 14   /* pass 1: G += (K_mn W^1/2)(K_mn W^1/2)^T, 2 N m^2 FLOP on the fp64 matrix cores */
#define GPMI_PROF_SGP_FACTOR 15 /* the m x m algebra: two factorisations, their inverses, H, c, the reductions */
#define GPMI_PROF_SGP_GRAD 16   /* the gradient: S, T, M2 and pass 2 (panel rebuild, T K_mn, the contractions: theta, and Z on request) */
/* gpmi_sgp_spatial_derivatives (tools/sparse_post_bench.py) books the cross build and its four products per panel under
 * GPMI_PROF_SGP_GRAM and the fused derivative kernel with its run sum under GPMI_PROF_SGP_GRAD; gpmi_sgp_posterior_draws
 * books Sigma under GPMI_PROF_DRAWS_SIGMA, and its tail books the classes of gpmi_posterior_draws. */
/* gpmi_lml_hessian books its four stages under the ids of the sparse model's (one handle runs one or the other) */
#define GPMI_PROF_HESS_BUILD GPMI_PROF_SGP_BUILD
#define GPMI_PROF_HESS_GEMM GPMI_PROF_SGP_GRAM
#define GPMI_PROF_HESS_TRACE GPMI_PROF_SGP_FACTOR
#define GPMI_PROF_HESS_CONTRACT GPMI_PROF_SGP_GRAD
/* the gpmi_ggp_* entry points (tools/generalised_bench.py) book under the same ids: the likelihood-terms kernel with its
 * totals, the K V products, the formation of B = I + sw sw^T o K, and the gradient's tail from the scaled solve to the
 * contraction (its many-right-hand-side solves are booked under GPMI_PROF_TRSM as well); the factorisations and the
 * triangular sweeps book their own classes (PANEL, SYRK*, FLOW, SOLVE) */
#define GPMI_PROF_GGP_TERMS GPMI_PROF_SGP_BUILD
#define GPMI_PROF_GGP_KV GPMI_PROF_SGP_GRAM
#define GPMI_PROF_GGP_BFORM GPMI_PROF_SGP_FACTOR
#define GPMI_PROF_GGP_GRAD GPMI_PROF_SGP_GRAD
#define GPMI_PROF_NCLASS 17
/* on = 0: off; 1: every class; otherwise a class bitmask shifted left by one (2 << klass) */
int gpmi_profile_enable(gpmi_ctx* ctx, int on);
/* accumulated since the last reset: launches, total ms, algorithmic flops and bytes */
int gpmi_profile_read(gpmi_ctx* ctx, int klass, int64_t* launches, double* ms, double* flops,
                      double* bytes);
int gpmi_profile_reset(gpmi_ctx* ctx);
/* shader clock (GHz) held during the stamped trailing-update launches since the last reset: cycles (s_memtime)
 * over wall time (s_memrealtime) of the first workgroups of every launch; 0 if nothing was stamped */
int gpmi_profile_clock(gpmi_ctx* ctx, double* ghz);

/* ---- device-pointer entry points (kernel tests / micro-benchmarks) -------------------
 * Matrices are row-major with a leading dimension ld of at least the row length and a multiple of 32 (the library's own
 * matrices have ld = n + 32, off a power-of-two pitch); m, n multiples of 128.  tests/test_kernels_gpu.py holds both entry
 * points to exact results on integer data, in the whole buffer. */
int gpmi_dev_alloc(gpmi_ctx* ctx, int64_t bytes, void** ptr_dev);
int gpmi_dev_free(gpmi_ctx* ctx, void* ptr_dev);
int gpmi_dev_upload(gpmi_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes);
int gpmi_dev_download(gpmi_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes);
/* in-place lower Cholesky of the n x n matrix at A_dev, of which only the tiles on and below the diagonal are read.  Untouched: the
 * columns from n on, every 128 x 128 tile strictly above the diagonal, and the part of tile (0, 0) above the diagonal.
 * The part above the diagonal inside the other diagonal tiles is workspace: the trailing updates write whole diagonal
 * tiles (or their two diagonal 64 x 64 quarters), so it returns holding intermediate values of theirs.
 * On a bare handle (no gpmi_set_data) the factorisation runs in stream order on the full chip at every n: the
 * flag-ordered tail and the look-ahead steps need the CU-masked stream pair, which only a handle whose data set has
 * np >= 5120 owns (the factor is the same bits either way; *info is the order of the first leading minor that fails, or
 * -6 if a poll of the flag-ordered launch gave up). */
int gpmi_dev_potrf(gpmi_ctx* ctx, double* A_dev, int64_t n, int64_t ld, int* info);
/* C (m x n, lower tiles only if lower != 0) -= A (m x k) * B (n x k)^T; k a multiple of 16, A and B may be one buffer.
 * lower != 0 (m >= n): every element on or below the diagonal is updated and no 128 x 128 tile strictly above it is
 * touched; above the diagonal inside a diagonal tile an element is either updated or left as it was (the 128 x 128
 * kernels update the whole tile, the 64 x 64 kernels its two diagonal quarters). */
int gpmi_dev_gemm_nt(gpmi_ctx* ctx, double* C_dev, int64_t ldc, const double* A_dev, int64_t lda,
                     const double* B_dev, int64_t ldb, int64_t m, int64_t n, int64_t k, int lower);

#ifdef __cplusplus
}
#endif
#endif /* GPMI_H */
