/* libgpt_hip — C ABI of the MI355X (gfx950) Gaussian-process transportation hot path.
 *
 * The reference (vyasakash231/gaussian_process_transportation) has no FFI for this path: its
 * boundary is the Python duck type consumed by PolicyTransportation
 * (policy_transportation/transportation/policy_transportation.py:12-14, 24, 30-32, 41-43) and
 * implemented by GaussianProcess (policy_transportation/models/gaussian_process.py:16-126) on
 * top of scikit-learn's GaussianProcessRegressor.  Each entry point below names the reference
 * call it stands in for; the ctypes binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no torch / numpy types; all matrices are C-contiguous row-major.  Fit inputs are always fp64;
 *     queries and outputs of the predict entry points are in the MODEL's element type: fp64 (double) unless the
 *     model was fitted with GPT_F32 (float) — see gpt_set_dtype / gpt_fit_svgp
 *   - "host" pointers are ordinary process memory, "dev" pointers are HIP device memory on the
 *     handle's device (e.g. torch.Tensor.data_ptr()); the library owns every other allocation
 *   - every function returns 0 on success or a negative GPT_E_* code; gpt_last_error() returns
 *     the message of the last failure on the calling thread
 *   - one handle = one fitted model on one GPU; a handle is not thread-safe, but different handles may be used from
 *     different threads at the same time (the hyper-parameter search drives its independent restarts that way)
 *   - D (input dims) in 1..15: D <= 3 (the reference's transport problems are 2-D and 3-D) is the tuned layout, D = 4..8 and
 *     9..15 run on wider source layouts (rows of 8 / 16) with the same entry points and results (the reference's regressor is
 *     dimension-agnostic; D > 15 is refused with GPT_E_ARG); O (outputs) >= 1; length_scale has 1 (isotropic) or D entries
 */
#ifndef GPT_HIP_H
#define GPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpt_handle gpt_handle;

#define GPT_OK 0
#define GPT_E_HIP (-1)        /* HIP runtime / launch failure                                   */
#define GPT_E_NOT_PD (-2)     /* non-positive pivot in the Cholesky: numpy.linalg.LinAlgError,  *
                               * as sklearn/gaussian_process/_gpr.py:348-358 raises             */
#define GPT_E_ARG (-3)        /* bad argument                                                   */
#define GPT_E_STATE (-4)      /* model not fitted / factor not committed                        */

/* Element type of a model's prediction side (scaled sources, alpha, packed inverse factor, queries, outputs).
 * The factorisation always runs in fp64; with GPT_F32 its results are rounded once when the model is packed and the
 * prediction kernels run on v_mfma_f32_16x16x4_f32 — the arithmetic of the reference's torch SVGP path
 * (models/torch/stocastic_variational_gaussian_process_derivatives.py computes in torch.float32). */
#define GPT_F64 0
#define GPT_F32 1

/* Number of visible HIP devices (0 when no GPU: the Python shim then refuses to run). */
int gpt_device_count(void);
/* Text of the last error on this thread ("" if none). */
const char* gpt_last_error(void);
/* Library version string. */
const char* gpt_version(void);

/* Create / destroy a model handle bound to `device`. */
int gpt_create(gpt_handle** out, int device);
void gpt_destroy(gpt_handle* h);
/* Launch all kernels of this handle on `hip_stream` (hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream); NULL restores the handle's own stream. */
int gpt_set_stream(gpt_handle* h, void* hip_stream);
/* Block until the handle's stream is idle. */
int gpt_synchronize(gpt_handle* h);

/* Element type of the models this handle fits from now on (default GPT_F64). */
int gpt_set_dtype(gpt_handle* h, int dtype);

/* (new) Derivatives (J, Jvar, d var) of Matern 3/2 and 5/2 models on this handle: 0 (default) refuses them with GPT_E_ARG, as
 * the reference's numbers for them are its RBF formulas applied to a Matern k*; 1 gives the analytic derivatives of the Matern
 * posterior (gpt_fit_kernel, gpt_derivative).  Per handle, kept across fits; no effect on RBF models, Matern 1/2 stays refused. */
int gpt_set_matern_derivatives(gpt_handle* h, int enable);

/* fit — replaces GaussianProcess.fit (models/gaussian_process.py:25-43) for fixed hyper-
 * parameters: sklearn's K = c*RBF(X/l) + (noise_level + alpha)*I, L = cholesky(K), alpha_ =
 * cho_solve(L, Y) (sklearn/_gpr.py:346-364) plus the factor of K^-1 the derivative code needs
 * (gaussian_process.py:42-43, kept here as W = L^-1).  X is (N,D), Y is (N,O), host memory; rows
 * with NaN must already be filtered by the caller (gaussian_process.py:33-35 does it in Python).
 * Returns GPT_E_NOT_PD when a pivot is <= 0. */
int gpt_fit(gpt_handle* h, const double* X, const double* Y, int64_t N, int D, int O,
            const double* length_scale, int n_ls, double constant_value, double noise_level,
            double alpha_jitter);

/* The same for `ConstantKernel * Matern(nu) + WhiteKernel` (sklearn/gaussian_process/kernels.py:1717-1778), the
 * kernel the reference's examples use for their dynamics GP (example/2D/surface_generalization.py:49,
 * example/3D/surface_generalization_3D.py:42).  gpt_fit == kernel_type GPT_KERNEL_RBF.  The derivative entry points
 * (J, Jvar, d var) give the analytic derivatives of this model's posterior for Matern 3/2 and 5/2:
 *   d k(x, X_n) / d x_d = c g(r) (X_n,d - x_d) / l_d^2,  g = 3 e^{-sqrt3 r} (3/2),  5/3 (1 + sqrt5 r) e^{-sqrt5 r} (5/2),
 * not the RBF coefficient the reference's gaussian_process.py:63-126 applies to any kernel — once enabled by
 * gpt_set_matern_derivatives (GPT_E_ARG before).  Matern 1/2 is not differentiable at the training points: GPT_E_ARG. */
#define GPT_KERNEL_RBF 0
#define GPT_KERNEL_MATERN12 1
#define GPT_KERNEL_MATERN32 2
#define GPT_KERNEL_MATERN52 3
int gpt_fit_kernel(gpt_handle* h, const double* X, const double* Y, int64_t N, int D, int O,
                   const double* length_scale, int n_ls, double constant_value, double noise_level,
                   double alpha_jitter, int kernel_type);

/* Exact-GP algebra on SVGP pseudo-points — the fit behind the reference's `convert_to_exact_gp`
 * (policy_transportation/models/torch/stocastic_variational_gaussian_process_derivatives.py:72-78):
 * K = c*k(X,X) + Sigma + alpha_jitter*I with a full SPD matrix Sigma (N,N) (the per-task pseudo-point covariance)
 * in place of the scalar noise; alpha = K^-1 Y.  One handle per task (O = 1, c = that task's outputscale).
 * Afterwards gpt_predict_all gives mean, var = c - k*^T K^-1 k* (k** carries no noise: :120-123), the Jacobian
 * and its variance c g(0)/l_d^2 - dk_d^T K^-1 dk_d (:132-153; g(0) as at gpt_derivative).  Host memory. */
int gpt_fit_noise_matrix(gpt_handle* h, const double* X, const double* Y, int64_t N, int D, int O,
                         const double* length_scale, int n_ls, double constant_value, const double* Sigma,
                         double alpha_jitter, int kernel_type);

/* The whole multi-task model of the reference's SVGP exact conversion in ONE handle — replaces
 * SVGP.convert_to_exact_gp (models/torch/stocastic_variational_gaussian_process_derivatives.py:72-78) and feeds
 * posterior_f (:113-129) / posterior_f_prime (:132-153):
 *   Z (N,D) inducing points; y (T,N) pseudo-targets; Sigma (T,N,N) SPD pseudo-point covariances; outputscale (T);
 *   length_scale (1 or D, shared by the tasks as in the reference's kernel, batch_shape [1]).
 * Per task t: K_t = outputscale_t RBF(Z,Z) + Sigma_t + jitter I, W_t = chol(K_t)^-1, alpha_t = K_t^-1 y_t (fp64).
 * The tasks' factors are stacked into one A operand (each times its outputscale) and share one generated B operand,
 * so a query pays its exps once, not T times.  Afterwards the predict entry points return, with O = T:
 *   mean (M,T); var (M,T) = outputscale_t - k*_t^T K_t^-1 k*_t; J (M,T,D); Jvar (M,T,D) = outputscale_t / l_d^2 -
 *   dk_d^T K_t^-1 dk_d   (the reference takes sqrt of both variances; the caller does).
 * dtype: GPT_F64 or GPT_F32 (BASELINE configs[4] is fp32).  T <= 32.  Host memory.  GPT_E_NOT_PD if a K_t is not PD. */
int gpt_fit_svgp(gpt_handle* h, const double* Z, const double* y, const double* Sigma, int64_t N, int D, int T,
                 const double* length_scale, int n_ls, const double* outputscale, double jitter, int dtype);

/* (new) Variational training of the SVGP transport model — replaces StocasticVariationalGaussianProcess.fit
 * (policy_transportation/models/torch/stocastic_variational_gaussian_process_derivatives.py:168-187: Adam, lr, over
 * gpytorch's VariationalELBO of the model at :15-63).  fp64 throughout, on `device`, host memory in and out.
 *   X (N,D), Y (N,T) training data (D 1..15, T 1..32); n_inducing Z 1..1024;
 *   in / out, updated in place: Z (Z,D) inducing points, m (T,Z) whitened variational means, C (T,Z,Z) variational
 *   Cholesky factors (lower triangle; the strict upper triangle is ignored and returned as passed), raw_lengthscale (D),
 *   raw_outputscale (T), raw_noise (T+1: per task, then the global noise) — softplus-constrained as gpytorch's defaults:
 *   l = softplus(raw), c_t = softplus(raw), noise_t = (1e-4 + softplus(raw_t)) + (1e-4 + softplus(raw_global));
 *   schedule: step s uses rows idx[batch_begin[s] .. batch_begin[s+1]) (1 .. 1024 rows; idx in [0,N)), n_steps >= 1;
 *   Adam (betas 0.9, 0.999, eps 1e-8) with learning rate lr, its state zero at the call; loss_trace (n_steps, may be NULL)
 *   receives each step's negative ELBO (before that step's update).
 * Every step is enqueued without a host round trip; the result is bit-reproducible.  GPT_E_NOT_PD (message: the optimiser
 * step) if chol(K(Z,Z) + 1e-4 I) meets a non-positive pivot — the parameters are then left as passed.  GPT_E_ARG for sizes
 * outside the limits above, an empty schedule or non-finite input. */
int gpt_svgp_train(int device, const double* X, const double* Y, int64_t N, int D, int T, int n_inducing, double* Z, double* m,
                   double* C, double* raw_lengthscale, double* raw_outputscale, double* raw_noise, const int64_t* idx, int64_t n_idx,
                   const int64_t* batch_begin, int64_t n_steps, double lr, double* loss_trace);

/* (new) One minibatch of the same objective without the update — the loss `-mll(output, y_batch)` and its `backward()` of
 * stocastic_variational_gaussian_process_derivatives.py:180-182: Xb (b,D), Yb (b,T), num_data = N of the KL term's 1/N;
 * parameters as at gpt_svgp_train (read only); loss (1) and the gradient of every raw parameter, each shaped like its
 * parameter (grad_C zero above the diagonal).  Gradient pointers may be NULL. */
int gpt_svgp_elbo_grad(int device, const double* Xb, const double* Yb, int64_t b, int64_t num_data, int D, int T, int n_inducing,
                       const double* Z, const double* m, const double* C, const double* raw_lengthscale, const double* raw_outputscale,
                       const double* raw_noise, double* loss, double* grad_Z, double* grad_m, double* grad_C,
                       double* grad_raw_lengthscale, double* grad_raw_outputscale, double* grad_raw_noise);

/* (new) Variational training of the point-cloud surface SVGP — replaces StocasticVariationalGaussianProcess.fit of
 * policy_transportation/models/torch/stocastic_variational_gaussian_process.py:68-89 (Adam on gpytorch's VariationalELBO
 * of the SVGP at :15-60).  The objective of gpt_svgp_train with a length-scale per task: raw_lengthscale (T,D),
 * K_t(Z,Z) = c_t k_{l_t}(Z,Z) + 1e-4 I.  Every other argument, the schedule, Adam and the failure contract as at
 * gpt_svgp_train; limits: n_inducing 1..4096, T 1..32, D 1..15, 1..1024 rows per batch.  Each task's Z x Z work runs
 * device-wide (blocked Cholesky + inverse, MFMA GEMMs); the result is bit-reproducible.
 * Failure: after a non-positive pivot every glue kernel returns at once, but the factor and GEMM launches of the steps
 * already enqueued still run (on stale data; no parameter changes), so a call that fails early costs about as long as
 * the whole schedule.
 * Memory, with NP = n_inducing rounded up to a multiple of 512: C is kept padded (NP x NP per task) in the parameters,
 * gradients and both Adam moments, so one call takes about 32 (T + 1) NP^2 bytes of device memory and 16 T NP^2 bytes of
 * host memory (T = 1, Z = 1000: 67 MB / 17 MB; T = 32, Z = 4096: 17.7 GB / 8.6 GB). */
int gpt_svgp_surface_train(int device, const double* X, const double* Y, int64_t N, int D, int T, int n_inducing, double* Z,
                           double* m, double* C, double* raw_lengthscale, double* raw_outputscale, double* raw_noise,
                           const int64_t* idx, int64_t n_idx, const int64_t* batch_begin, int64_t n_steps, double lr,
                           double* loss_trace);

/* (new) One minibatch of the surface objective without the update — `loss = -self.mll(output, y_batch)` and its
 * `loss.backward()` at stocastic_variational_gaussian_process.py:84-87.  Arguments as at gpt_svgp_elbo_grad, with
 * raw_lengthscale and grad_raw_lengthscale shaped (T,D).  Gradient pointers may be NULL. */
int gpt_svgp_surface_elbo_grad(int device, const double* Xb, const double* Yb, int64_t b, int64_t num_data, int D, int T,
                               int n_inducing, const double* Z, const double* m, const double* C, const double* raw_lengthscale,
                               const double* raw_outputscale, const double* raw_noise, double* loss, double* grad_Z,
                               double* grad_m, double* grad_C, double* grad_raw_lengthscale, double* grad_raw_outputscale,
                               double* grad_raw_noise);

/* (new) The variational predictive of the surface SVGP — replaces `self.gp(x)` in StocasticVariationalGaussianProcess.predict
 * (stocastic_variational_gaussian_process.py:95-103) and the jacobian of its mean in derivative (:105-111).  Per task,
 * with a = W_t c_t k_{l_t}(Z, x), W_t = chol(c_t k(Z,Z) + 1e-4 I)^-1: mean (M,T) = a^T m_t; var (M,T, may be NULL) =
 * c_t - |a|^2 + |C_t^T a|^2 (the latent f, no likelihood noise); J (M,T,D, may be NULL) = d mean / d x.  fp64, host
 * memory in and out.  GPT_E_NOT_PD if a factor meets a non-positive pivot.  Memory: about 8 (3 NP^2 + 3072 NP) bytes of
 * device and 16 NP^2 bytes of host memory (NP as at gpt_svgp_surface_train), plus the inputs and outputs. */
int gpt_svgp_surface_predict(int device, const double* Z, const double* m, const double* C, const double* raw_lengthscale,
                             const double* raw_outputscale, int n_inducing, int D, int T, const double* Xq, int64_t M,
                             double* mean, double* var, double* J);

/* (new) Greedy active-learning subset selection — replaces the selection loop of the reference's large-input regressor
 * (policy_transportation/models/gaussian_process_al.py:26-57: start from an initial subset, then repeatedly add the pool
 * point whose posterior standard deviation is largest and refit) for FIXED hyper-parameters, where that loop is a pivoted
 * Cholesky factorisation of the pool's kernel matrix with the diagonal pivot rule.  fp64, on `device`, host memory.
 *   X (N,D) pool, D 1..15; length_scale (D); c constant_value; noise the WhiteKernel level; alpha the jitter;
 *   kernel_type GPT_KERNEL_*; initial (n_initial distinct pool indices, may be NULL when n_initial == 0): the first pivots,
 *   prescribed in this order; n_total: points to select in all (n_initial <= n_total <= N);
 *   selected (n_total): pool indices in insertion order (the initial ones first); selection_variance (n_total - n_initial):
 *   the posterior variance of each chosen point when it was chosen, in sklearn's convention (kernel diagonal with the white
 *   noise, minus |L^-1 k*|^2: sklearn/gaussian_process/_gpr.py:472-494), i.e. the square of the std the reference takes
 *   its argmax over; residual_variance (N, may be NULL): the same variance of every pool point after the last insertion.
 * Ties go to the lowest pool index (numpy.argmax over the reference's order-preserving pool).  The whole schedule is
 * enqueued without a host round trip; the result is bit-reproducible.  One insertion streams the pool factor (N x j
 * doubles), so a call reads about 4 N n_total^2 bytes of device memory.
 * GPT_E_NOT_PD: a pivot's variance + alpha was not positive (outputs untouched).  GPT_E_ARG: sizes outside the limits
 * above, a repeated or out-of-range initial index, NaN / infinity in the pool, or device buffers (the pool factor, 8 N n_total
 * bytes, plus the pool, its scaled copy and the per-point state) above 80 % of the device's free memory at the call. */
int gpt_select_greedy(int device, const double* X, int64_t N, int D, const double* length_scale, double c, double noise,
                      double alpha, int kernel_type, const int64_t* initial, int n_initial, int n_total, int64_t* selected,
                      double* selection_variance, double* residual_variance);

/* (new) A batch of independent small exact GPs, each handled by one workgroup and the whole batch by one launch per operation
 * and size class (n <= 32, n <= 128) — the three entry points below.  They share:
 *   layout: B models, ragged.  X (sum n_b, D) and Y (sum n_b, O) are the models' rows concatenated, n_begin (B + 1) their
 *   offsets (n_begin[0] = 0); queries Xq (sum M_b, D) with q_begin (B + 1) likewise, outputs concatenated by the same offsets;
 *   hyper-parameters per model: length_scale (B, n_ls), n_ls 1 or D for the whole batch, constant_value (B), noise_level (B);
 *   alpha_jitter and kernel_type (GPT_KERNEL_*) are shared.  fp64, on `device`, host memory in and out.
 *   limits (GPT_E_ARG, the message names the limit): 1 <= n_b <= 128, D 1..15, O 1..16, 1 <= B <= 2^20, M_b >= 0 and
 *   sum M_b < 2^31, increasing offsets, no NaN / infinity, length_scale and constant_value > 0, noise_level >= 0.
 *   status (B): GPT_OK, or GPT_E_NOT_PD for a model whose Cholesky met a pivot <= 0 (sklearn's LinAlgError); that model's
 *   outputs are left untouched and every other model is computed as usual.  The return value is GPT_OK whenever the batch ran.
 *   Every sum over a model's points runs in a fixed order: a model's results do not depend on the batch around it, and a
 *   query's not on the other queries, bit for bit.
 *
 * gpt_batch_lml_objective — log_marginal_likelihood(theta, eval_gradient=True) (sklearn/_gpr.py:537-652) for B (data, theta)
 * pairs at once: what the optimiser of every GaussianProcess.fit in the reference's per-frame loop
 * (example/comparisons/multi_reference_frames/models/model_gpt.py:74-83, a transport fitted on 10 points per frame pair)
 * evaluates a few hundred times.  lml (B); grad (B, 2 + n_ls) with respect to log [c, l.., noise], as gpt_lml_objective;
 * all four kernel types. */
int gpt_batch_lml_objective(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                            const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                            double alpha_jitter, int kernel_type, double* lml, double* grad, int* status);

/* (new) gpt_batch_fit — GaussianProcess.fit at fixed hyper-parameters (models/gaussian_process.py:25-43 ->
 * sklearn/_gpr.py:346-364) for every model of the batch, the fits of model_gpt.py:74-83 in one call: L (sum n_b^2: each
 * model's n_b x n_b factor, zeros above the diagonal; may be NULL), alpha (sum n_b, O), lml (B; may be NULL). */
int gpt_batch_fit(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                  const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                  double alpha_jitter, int kernel_type, double* L, double* alpha, double* lml, int* status);

/* (new) gpt_batch_predict — the fused posterior of every model at its own queries: GaussianProcess.predict and .derivative
 * (gaussian_process.py:46-55, 63-102) and .derivative_of_variance (:104-126) as model_gpt.py:74-83 calls them per frame.
 * Stateless: the models are factored again inside the call (microseconds at these sizes).  Any output may be NULL:
 * mean (sum M, O); var (sum M) = max(c + noise - |W k*|^2, 0) as gpt_predict; J (sum M, O, D); Jvar (sum M, D) = c / l_d^2 -
 * |W dk_d|^2; dvar (sum M, D) = -2 (W dk_d).(W k*), W = L^-1.  J, Jvar and dvar are RBF only (GPT_E_ARG on a Matern batch).
 * Device memory: the inputs and outputs plus 4 n_b (n_b + 1) bytes per model. */
int gpt_batch_predict(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O,
                      const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                      double alpha_jitter, int kernel_type, const double* Xq, const int64_t* q_begin, double* mean, double* var,
                      double* J, double* Jvar, double* dvar, int* status);

/* (new) gpt_batch_optimize — the hyper-parameter search of such a batch on the device: R runs, run r maximising the LML of model
 * run_model[r] (0 .. B - 1) over theta = log [c, l.., noise] from theta0[r] (R, 2 + n_ls) inside `bounds` (2 + n_ls, 2: lo, hi
 * in log space, finite; lo == hi fixes a component; a start outside its bounds is clipped).  One workgroup carries one run
 * through a projected BFGS iteration with a backtracking line search (csrc/gpt_batch_opt.hip states it), evaluating the
 * objective of gpt_batch_lml_objective in place; a launch spends at most evals_per_launch evaluations per run, then the host
 * reads the R status words and launches again for the runs still live.  A run's five outputs do not depend on the other runs,
 * on their order or on evals_per_launch, bit for bit.  The restarts of sklearn's protocol are runs of one model: the caller
 * keeps the best.  pgtol, ftol, max_iter, max_evals: as scipy's L-BFGS-B (sklearn passes 1e-5, 2.22e-9, 15000, 15000).
 * Outputs: theta (R, 2 + n_ls), lml (R), iterations (R), evaluations (R), status (R) GPT_OPT_*.  A run whose start is not PD
 * has status GPT_OPT_NOT_PD_START, lml = -infinity and the clipped start in theta.  Limits (GPT_E_ARG, the message names the
 * limit): those of gpt_batch_lml_objective, 1 <= R <= 2^20, run_model in [0, B), no NaN / infinity, lo <= hi, tolerances and
 * caps > 0.  The return value is GPT_OK whenever the batch ran: a run that did not converge says so in its status.  Device
 * memory: the inputs and 8 ((2 + n_ls)^2 + 7 (2 + n_ls) + 7) bytes per run. */
#define GPT_OPT_PGTOL 0        /* projected gradient <= pgtol                                  */
#define GPT_OPT_FTOL 1         /* relative decrease of an accepted step <= ftol                */
#define GPT_OPT_MAX_ITER 2     /* iteration cap                                                */
#define GPT_OPT_MAX_EVALS 3    /* evaluation cap                                               */
#define GPT_OPT_LINESEARCH 4   /* no acceptable step after 30 halvings                         */
#define GPT_OPT_NOT_PD_START 5 /* the (clipped) start point's matrix is not positive definite */
int gpt_batch_optimize(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O, int n_ls,
                       const int* run_model, const double* theta0, int64_t R, const double* bounds, double alpha_jitter,
                       int kernel_type, double pgtol, double ftol, int max_iter, int max_evals, int evals_per_launch, double* theta,
                       double* lml, int* iterations, int* evaluations, int* status);

/* (new) gpt_batch_optimize_bounded — gpt_batch_optimize with a box per run: run_bounds (R, 2 + n_ls, 2) in place of `bounds`, run r
 * searching inside run_bounds[r] (the same checks per run: finite, lo <= hi, the start clipped to the run's own box).  It is the
 * same kernel reading `bounds + run * stride` (gpt_batch_optimize: stride 0), so a run's five outputs equal, bit for bit, those of
 * gpt_batch_optimize called with that run's box as the shared one, whatever the other runs, their order or evals_per_launch.
 * For searches whose candidates differ in their bounds, e.g. a ceiling on the length-scale per candidate
 * (GaussianProcessTransportationDiffeo.optimize_diffeomorphism).  Device memory: 16 (2 + n_ls) bytes per run more. */
int gpt_batch_optimize_bounded(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D, int O, int n_ls,
                               const int* run_model, const double* theta0, int64_t R, const double* run_bounds, double alpha_jitter,
                               int kernel_type, double pgtol, double ftol, int max_iter, int max_evals, int evals_per_launch,
                               double* theta, double* lml, int* iterations, int* evaluations, int* status);

/* (new) gpt_batch_fold_scan — does the displacement map x -> x + psi_b(x) of each of B small GPs fold, and how badly does the
 * reference's inverse surrogate undo it: the scoring of policy_transportation/transportation/
 * gaussian_process_transportation_diffeomorphic.py (check_invertibility :109-121, diffeomorphism_error :123-137) for B candidate
 * models in one call, reduced on the device to five numbers per model.  Layout, limits and status as the batch family above
 * (ragged models, 1 <= n_b <= 128, fp64, hyper-parameters per model), with O = D <= 3 (Y (sum n_b, D): a displacement) and RBF
 * only (GPT_E_ARG on a Matern batch, as the derivatives of gpt_batch_predict).  Queries: q_begin == NULL: every model scans the
 * same M queries Xq (M, D) and the per-query outputs are (B, M, ..); otherwise ragged as gpt_batch_predict (q_begin (B + 1),
 * M = q_begin[B] ignored).  B M_b summed < 2^31.
 *   per model: K(X_b) factored, alpha = K^-1 Y_b; surrogate != 0: also the GP on inputs X_b + Y_b (rounded to fp64) with targets
 *   -Y_b at the same hyper-parameters (:115-117), beta = K(X_b + Y_b)^-1 (-Y_b);
 *   per query x: psi = k(x, X_b) alpha, J = d psi / d x, det = det(I + J) (closed form), z = x + psi; with the surrogate
 *   err = |psi + k(z, X_b + Y_b) beta|_2 (:118-120);
 *   per model: min_det (B), argmin (B; the lowest query index attaining it), n_fold (B; queries with det <= 0), err_sum (B; the
 *   reference's number), err_max (B).  A model without queries: +infinity, -1, 0, 0, 0.
 *   det (sum M_b), z (sum M_b, D), err (sum M_b): optional (NULL).
 * status (B): GPT_E_NOT_PD: all of the model's outputs stay untouched.  surrogate_status (B): the same for the surrogate's
 * matrix; then err, err_sum and err_max stay untouched, everything else is computed.  surrogate == 0: err, err_sum, err_max and
 * surrogate_status are not touched and may be NULL.  The return value is GPT_OK whenever the batch ran.
 * A query's det, z and err do not depend on the other queries or the batch; a model's five numbers do not depend on the batch
 * around it nor on which optional arrays are asked for: every sum and minimum runs in an order fixed by (n_b, D, M_b), bit for bit.
 * Device memory: the inputs, 16 n_b D bytes per model, 32 bytes per 64 queries, and the optional arrays. */
int gpt_batch_fold_scan(int device, const double* X, const double* Y, const int64_t* n_begin, int64_t B, int D,
                        const double* length_scale, int n_ls, const double* constant_value, const double* noise_level,
                        double alpha_jitter, int kernel_type, const double* Xq, const int64_t* q_begin, int64_t M, int surrogate,
                        double* min_det, int64_t* argmin, int64_t* n_fold, double* err_sum, double* err_max, double* det, double* z,
                        double* err, int* status, int* surrogate_status);

/* predict — replaces GaussianProcess.predict (gaussian_process.py:46-55 -> sklearn/_gpr.py:441-494).
 * mean (M,O); var (M,) = max(c + noise_level - |L^-1 k*|^2, 0) (the caller applies sqrt, the
 * tiling over O and the reference's `- sqrt(noise_level)` quirk).  var may be NULL. Host memory. */
int gpt_predict(gpt_handle* h, const void* Xq, int64_t M, void* mean, void* var);

/* derivative — replaces GaussianProcess.derivative (gaussian_process.py:63-102).
 * J (M,O,D) with J[m,o,d] = d mean_o / d x_d; Jvar (M,D) = c g(0)/l_d^2 - dk_d^T K^-1 dk_d (the
 * reference tiles it over O), g(0) = 1 (RBF), 3 (Matern 3/2), 5/3 (Matern 5/2): the prior variance of the
 * derivative, -d^2 k / d tau_d^2 at tau = 0.  Jvar may be NULL.  Host memory.  Matern 3/2 / 5/2 models: GPT_E_ARG unless
 * gpt_set_matern_derivatives enabled them; Matern 1/2: GPT_E_ARG. */
int gpt_derivative(gpt_handle* h, const void* Xq, int64_t M, void* J, void* Jvar);

/* derivative_of_variance — replaces GaussianProcess.derivative_of_variance
 * (gaussian_process.py:104-126).  g is (D,M).  Host memory. */
int gpt_dvariance(gpt_handle* h, const void* Xq, int64_t M, void* g);

/* Fused metric path: any of mean (M,O) / var (M,) / J (M,O,D) / Jvar (M,D) / dvar (D,M) may be
 * NULL (multi-task model: var (M,T), Jvar (M,T,D), no dvar).  Buffers in the model's element type.
 * Host memory (pageable is fine); queries are streamed through the device in chunks of 131072, the outputs of
 * one chunk leaving on a copy stream while the next chunk computes.  Returns when every output is in place. */
int gpt_predict_all(gpt_handle* h, const void* Xq, int64_t M, void* mean, void* var,
                    void* J, void* Jvar, void* dvar);
/* Same with every pointer in device memory; asynchronous on the handle's stream. */
int gpt_predict_all_dev(gpt_handle* h, const void* Xq_dev, int64_t M, void* mean_dev,
                        void* var_dev, void* J_dev, void* Jvar_dev, void* dvar_dev);
/* (new) Allocates the library-owned scratch a gpt_predict_all_dev call with M queries will use (grow-only; with
 * jacobian_variance != 0 for the 4-column path), so that the first such call does not allocate. */
int gpt_reserve(gpt_handle* h, int64_t M, int jacobian_variance);

/* (new) Inverse of the displacement map: for each of M targets y (M,D) the z with  z + mean(z) = y,  mean the posterior mean
 * of gpt_predict — the map of PolicyTransportation.transport (transportation/policy_transportation.py:30-35) after its affine
 * part, taken backwards.  The reference has no inverse: example/2D/surface_generalization_heteroschedastic _inverse_mapping.py:88-127
 * fits a SECOND transport with source and target swapped and walks a grid through it in a Python loop, and
 * GaussianProcessTransportationDiffeo.check_invertibility (transportation/gaussian_process_transportation_diffeomorphic.py:109-121)
 * measures how far that surrogate misses.  Here the equation itself is solved, damped Newton, every query in one wave of ONE launch:
 *   z <- Z0 (y when Z0 is NULL); r = z + mean(z) - y; A = I + J(z); rho = |r|_2; tol = rtol (1 + |y|_2); t = 1; passes = 1; repeat:
 *     rho <= tol -> GPT_INV_CONVERGED;  passes == max_passes -> GPT_INV_MAX_PASSES;  |det A| <= 2^-40 |A|_F^D -> GPT_INV_SINGULAR;
 *     z' = z - t A^-1 r, one more pass there; rho' < rho: z' is accepted and t = min(1, 2t); else t = t/2 and below 2^-20
 *     -> GPT_INV_STALLED.
 * Z (M,D): the last accepted point; residual (M): rho there; det (M): det(I + J) there — <= 0 where the map folds, the honest
 * form of the "locally diffeomorphic?" print of policy_transportation.py:52; passes (M): contractions over the sources spent;
 * status (M): GPT_INV_*.  residual, det and passes may be NULL.  A query's result does not depend on M or on the other queries,
 * bit for bit.  The return value is GPT_OK whenever the launch ran: a query that did not converge says so in its status.
 * GPT_E_STATE: no model.  GPT_E_ARG (the message names the limit): D != O or D > 3; a GPT_F32 or multi-task (gpt_fit_svgp) model;
 * Matern 1/2, or Matern 3/2 / 5/2 without gpt_set_matern_derivatives; rtol <= 0; max_passes < 1; M < 0 or M >= 2^31.  M = 0 does
 * nothing.  Device memory, asynchronous on the handle's stream; the model and the handle's scratch are left as they were. */
#define GPT_INV_CONVERGED 0
#define GPT_INV_MAX_PASSES 1
#define GPT_INV_SINGULAR 2
#define GPT_INV_STALLED 3
int gpt_inverse_map_dev(gpt_handle* h, const double* Y_dev, const double* Z0_dev, int64_t M, double rtol, int max_passes,
                        double* Z_dev, double* residual_dev, double* det_dev, int* passes_dev, int* status_dev);
/* (new) The same with every pointer in host memory (the 100 x 100 grid of the inverse-mapping example :110-127, the trajectory of
 * check_invertibility :109-121); also GPT_E_ARG for NaN / infinity in Y or Z0.  The device images belong to the handle.  Returns
 * when every output is in place. */
int gpt_inverse_map(gpt_handle* h, const double* Y, const double* Z0, int64_t M, double rtol, int max_passes, double* Z,
                    double* residual, double* det, int* passes, int* status);

/* (new) Transport of a demonstration in one device call: what PolicyTransportation.transport / transport_velocity /
 * transport_orientation (transportation/policy_transportation.py:30-75) compute on the host around three posterior calls — the
 * affine part, the posterior (the launches of gpt_predict_all_dev, unchanged), and the push-forward of positions, velocities and
 * orientations.  All arrays fp64.  Inputs: pos (M,D); the affine part gamma(x) = scale R (x - c_src) + c_dst with R (D,D)
 * row-major, c_src (D), c_dst (D); R_jac (D,D), the Jacobian of gamma as the caller defines it (the reference passes the
 * UNSCALED rotation, affine_trasformation.py:55-57); vel (M,D) or NULL; ori (M,4) as w,x,y,z or NULL.  Outputs, each of which may
 * be NULL except pos_out:
 *   pos_rot (M,D)  = gamma(pos)
 *   pos_out (M,D)  = gamma(pos) + mean(gamma(pos))
 *   var     (M)    raw, as gpt_predict's (the caller applies sqrt, the `- sqrt(noise_level)` quirk and the tiling)
 *   vel_out (M,D)  = (I + J(gamma pos)) R_jac vel
 *   vel_var (M)    = sum_d Jvar_d(gamma pos) (R_jac vel)_d^2, the same for every output (the caller tiles it)
 *   det_vel (M)    = det((I + J(gamma pos)) R_jac)
 *   ori_out (M,4)  = q(J') (x) ori, J' = (I + J(pos)) R_jac at the UN-rotated positions as the reference's transport_orientation
 *                    (:62); q: Bar-Itzhack's quaternion of the rotation closest to J', the dominant eigenvector of the
 *                    symmetric 4 x 4 matrix K(J') (six sweeps of cyclic Jacobi, column of the largest diagonal entry, lowest
 *                    index on a tie, normalised), sign fixed to w >= 0 before the product
 *   det_ori (M)    = det J'
 *   ori_gap (M)    = (lambda_4 - lambda_3) / |K|_F; where it is 0 the closest rotation is not unique and ori_out is one of several
 *   post_mean (M,D), post_J (M,D,D), post_Jvar (M,D) at gamma(pos) and post_J_ori (M,D,D) at pos: the posterior the epilogue
 *                    consumed (the reference keeps them as attributes)
 * GPT_E_STATE: no model.  GPT_E_ARG (the message names the limit): D != O or D > 3; ori, ori_out or ori_gap with D != 3; a GPT_F32
 * or multi-task (gpt_fit_svgp) model; Matern 1/2, or Matern 3/2 / 5/2 without gpt_set_matern_derivatives; M < 0 or M >= 2^31;
 * vel_out or vel_var without vel, ori_out without ori; a NULL among pos, pos_out, R, c_src, c_dst, R_jac.  M = 0 does nothing.
 * Device memory (the affine part too), asynchronous on the handle's stream; what the epilogue reads and the caller did not ask
 * for lives in scratch of the handle (grow-only).  The model and the results of later gpt_predict_all calls are left as they were. */
int gpt_transport_policy_dev(gpt_handle* h, const double* pos_dev, int64_t M, const double* R_dev, const double* c_src_dev,
                             const double* c_dst_dev, double scale, const double* R_jac_dev, const double* vel_dev,
                             const double* ori_dev, double* pos_rot_dev, double* pos_out_dev, double* var_dev, double* vel_out_dev,
                             double* vel_var_dev, double* det_vel_dev, double* ori_out_dev, double* det_ori_dev, double* ori_gap_dev,
                             double* post_mean_dev, double* post_J_dev, double* post_Jvar_dev, double* post_J_ori_dev);
/* (new) The same with every pointer in host memory; also GPT_E_ARG for NaN / infinity in pos, vel, ori or the affine part.  The
 * queries are streamed through the device in chunks of 131072 as gpt_predict_all's, the outputs of one chunk leaving on the copy
 * stream while the next computes; only the arrays asked for cross the bus.  Returns when every output is in place. */
int gpt_transport_policy(gpt_handle* h, const double* pos, int64_t M, const double* R, const double* c_src, const double* c_dst,
                         double scale, const double* R_jac, const double* vel, const double* ori, double* pos_rot, double* pos_out,
                         double* var, double* vel_out, double* vel_var, double* det_vel, double* ori_out, double* det_ori,
                         double* ori_gap, double* post_mean, double* post_J, double* post_Jvar, double* post_J_ori);

/* (new) The transported POLICY at points of the target scene that are not on the demonstration (a robot's position, the grid of a
 * stream plot): the source dynamics pulled back through the transport,
 *     x = Phi^-1(y),   v(y) = J_Phi(x) f(x),   Phi = gamma + psi o gamma.
 * The reference reaches this only by refitting a second GP on the moved demonstration (example/2D/surface_generalization.py:81-88)
 * and a third for its uncertainty (example/2D/surface_generalization_heteroschedastic_uncertainty.py:150-175).  h_map: the fitted
 * displacement model psi; h_dyn: a second fitted model, the dynamics f, with the same D; gamma(x) = scale R (x - c_src) + c_dst and
 * R_jac as in gpt_transport_policy.  All arrays fp64 except passes and status (int).  Inputs: y (M,D); x0 (M,D) guesses of the
 * preimages, or NULL; rtol, max_passes as gpt_inverse_map; std_offset.  Per point:
 *   z            the damped Newton iteration of gpt_inverse_map on z + psi(z) = y, started at gamma(x0) (at y when x0 is NULL):
 *                the same accept / reject rule, statuses, passes, residual and det = det(I + J_psi(z))
 *   x     (M,D)  = (z - c_dst) R / scale + c_src
 *   f     (M,D)  = mean of h_dyn at x
 *   vel   (M,D)  = A R_jac f,  A = I + J_psi(z) of the last accepted pass
 *   det, residual (M), passes, status (M, int; GPT_INV_*)
 *   var_dyn (M)      raw posterior variance of h_dyn at x, as gpt_predict's
 *   map_var (M)      raw posterior variance of h_map at z
 *   vel_var_map (M)    = sum_d Jvar_d(z) (R_jac f)_d^2, what gpt_transport_policy calls vel_var
 *   vel_var_dyn (M,D)  = s^2 sum_j (A R_jac)[i,j]^2,  s = sqrt(var_dyn) - std_offset: the std of the dynamics as the Python
 *                      predict returns it (std_offset = sqrt(noise_level)) pushed through J_Phi
 *   post_z (M,D), post_A (M,D,D), post_Jvar (M,D): z, A and the Jacobian variance of h_map at z, what the later stages consumed
 * Every output may be NULL except vel and status.  A point whose iteration does not converge still gets every output, at the z
 * it reached, and says so in its status.  x, f, vel, det, residual, passes, status, post_z and post_A come from ONE launch, one
 * wave per query (k_pullback_velocity); a query's values there do not depend on M or on the other queries, bit for bit.  The
 * variances come from the unchanged variance launches of the two handles (map_var and the Jacobian variance together: one pass of
 * the 4-column launch; the Jacobian variance alone: the 3-column one) and a one-thread-per-query epilogue.
 * GPT_E_STATE: a handle without a model.  GPT_E_ARG (the message names the limit): a NULL handle; h_map == h_dyn; handles on
 * different devices; different D; D != O or D > 3, a GPT_F32 or multi-task (gpt_fit_svgp) model, on either handle; a Matern 1/2
 * map, or a Matern 3/2 / 5/2 map without gpt_set_matern_derivatives (the dynamics may be any of the four kernels: it is only
 * evaluated); rtol <= 0 or NaN; max_passes < 1; M < 0 or M >= 2^31; a NULL among y, vel, status, R, c_src, c_dst, R_jac.  M = 0
 * does nothing.
 * Device memory (the affine part too).  Asynchronous: enqueued on h_map's stream, which first waits for what h_dyn's stream holds
 * so far; the variance of h_dyn runs on h_dyn's own stream (its workspace belongs to it) between two events, and h_dyn's stream
 * goes on only after its model has been read.  No host synchronisation; correct for the handles' own streams and after
 * gpt_set_stream on either.  Scratch and events belong to h_map (grow-only).  Both models are left as they were. */
int gpt_pullback_policy_dev(gpt_handle* h_map, gpt_handle* h_dyn, const double* y_dev, const double* x0_dev, int64_t M,
                            const double* R_dev, const double* c_src_dev, const double* c_dst_dev, double scale, const double* R_jac_dev,
                            double rtol, int max_passes, double std_offset, double* x_dev, double* vel_dev, double* f_dev,
                            double* det_dev, double* residual_dev, int* passes_dev, int* status_dev, double* var_dyn_dev,
                            double* map_var_dev, double* vel_var_map_dev, double* vel_var_dyn_dev, double* post_z_dev,
                            double* post_A_dev, double* post_Jvar_dev);
/* (new) The same with every pointer in host memory; also GPT_E_ARG for NaN / infinity in y, x0, the affine part or std_offset.
 * The queries are streamed through the device in chunks of 131072 as gpt_transport_policy's, through two staging sets of h_map;
 * only the arrays asked for cross the bus.  Returns when every output is in place. */
int gpt_pullback_policy(gpt_handle* h_map, gpt_handle* h_dyn, const double* y, const double* x0, int64_t M, const double* R,
                        const double* c_src, const double* c_dst, double scale, const double* R_jac, double rtol, int max_passes,
                        double std_offset, double* x, double* vel, double* f, double* det, double* residual, int* passes, int* status,
                        double* var_dyn, double* map_var, double* vel_var_map, double* vel_var_dyn, double* post_z, double* post_A,
                        double* post_Jvar);

/* (new) The transported policy through a CHAIN of transports, Phi = Phi_{K-1} o ... o Phi_0 (the reference's obstacle example moves
 * a demonstration twice, example/2D/surface_generalization_with_obstacle.py:142-200, and refits a GP on the result):
 *     x = Phi^-1(y),   v(y) = J_Phi(x) f(x),   Phi_k = gamma_k + psi_k o gamma_k.
 * stages: a HOST array of K entries, 1 <= K <= GPT_CHAIN_MAX, in the order the transports are applied (stage 0 first); each names
 * a handle with the fitted displacement model psi_k and gamma_k(x) = scale R (x - c_src) + c_dst with R_jac, as
 * gpt_pullback_policy's.  h_dyn: the dynamics f.  All models share one D.  Inputs: y (M,D); x0 (M,D) guesses of the SOURCE-space
 * preimages, or NULL; rtol, max_passes, std_offset as gpt_pullback_policy.  Per point:
 *   starts       with x0: g_0 = x0, g_{k+1} = gamma_k(g_k) + mean_k(gamma_k(g_k)); stage k's iteration starts at gamma_k(g_k).
 *                Without x0 every stage starts at its own y_k.
 *   stages K-1 .. 0:  y_{K-1} = y; z_k: the damped Newton iteration of gpt_pullback_policy on z + psi_k(z) = y_k (the same accept /
 *                reject rule, statuses, passes, residual, det); x_k = (z_k - c_dst) R / scale + c_src; y_{k-1} = x_k.  A stage that
 *                does not converge hands on the point it reached and says so; the stages before it still run.
 *   x     (M,D)  = x_0, the source-space preimage
 *   f     (M,D)  = mean of h_dyn at x
 *   vel   (M,D)  = B_{K-1} ... B_0 f,  B_k = A_k R_jac,k,  A_k = I + J_psi_k(z_k) of stage k's last accepted pass
 *   status (M, int)   the GPT_INV_* of the first stage in solve order (K-1 first) that is not CONVERGED, else CONVERGED
 *   var_dyn (M)       raw posterior variance of h_dyn at x
 *   vel_var_map (M,D) = sum_k sigma_k^2 sum_j (B_{K-1} ... B_{k+1})[i,j]^2,  sigma_k^2 = sum_d Jvar_k,d(z_k) (R_jac,k v_{k-1})_d^2,
 *                     v_{-1} = f, v_k = B_k v_{k-1}: each map's Jacobian variance pushed, to first order, through the maps after it
 *   vel_var_dyn (M,D) = s^2 sum_j (B_{K-1} ... B_0)[i,j]^2,  s = sqrt(var_dyn) - std_offset
 *   stage-major per-stage arrays, stage k's rows contiguous: stage_x (K,M,D), stage_z (K,M,D), stage_A (K,M,D,D), stage_Jvar
 *   (K,M,D) the Jacobian variance of psi_k at z_k, stage_map_var (K,M) the raw posterior variance of psi_k at z_k, stage_status,
 *   stage_passes (K,M, int), stage_residual, stage_det (K,M)
 * Every output may be NULL except vel and status.  For K = 1, x, vel, f, status and the stage arrays are gpt_pullback_policy's x,
 * vel, f, status, x, post_z, post_A, post_Jvar, map_var, status, passes, residual, det, and every column of vel_var_map its scalar.
 * x, f, vel, status and the stage arrays but Jvar and map_var come from ONE launch, one wave per query (k_chain_velocity); a
 * query's values there do not depend on M or on the other queries, bit for bit.  The variances come from the unchanged variance
 * launches of the handles, only those whose outputs were asked for, and a one-thread-per-query epilogue.
 * GPT_E_STATE: a handle without a model.  GPT_E_ARG (the message names the limit and the stage): K < 1 or K > GPT_CHAIN_MAX; stages
 * NULL; a NULL handle or a NULL R, c_src, c_dst, R_jac in a stage; h_dyn NULL; one handle twice among the stages and h_dyn; handles
 * on different devices or with different D; per handle what gpt_pullback_policy refuses of its map (every stage) and of its
 * dynamics; rtol <= 0 or NaN; max_passes < 1; M < 0 or M >= 2^31; a NULL among y, vel, status.  M = 0 does nothing.
 * Device memory (the affine parts too; the stages array itself is host memory and is not kept).  Asynchronous: enqueued on the
 * stream of stages[K-1].h, which first waits for what the other handles' streams hold so far; each variance launch runs on its own
 * handle's stream between two events, one after the other (each fills the device), and the other streams go on only after
 * their models have been read.  No host synchronisation.  Scratch, staging and events belong to stages[K-1].h (grow-only).  Every model is left as it was. */
#define GPT_CHAIN_MAX 4
typedef struct {
    gpt_handle* h;
    const double *R, *c_src, *c_dst, *R_jac;
    double scale;
} gpt_chain_stage;
int gpt_pullback_chain_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y_dev, const double* x0_dev, int64_t M,
                           double rtol, int max_passes, double std_offset, double* x_dev, double* vel_dev, double* f_dev,
                           int* status_dev, double* var_dyn_dev, double* vel_var_map_dev, double* vel_var_dyn_dev, double* stage_x_dev,
                           double* stage_z_dev, double* stage_A_dev, double* stage_Jvar_dev, double* stage_map_var_dev,
                           int* stage_status_dev, int* stage_passes_dev, double* stage_residual_dev, double* stage_det_dev);
/* (new) The same with every data pointer in host memory; also GPT_E_ARG for NaN / infinity in y, x0, an affine part, rtol or
 * std_offset.  The queries are streamed through the device in chunks of 131072 as gpt_pullback_policy's, through two staging sets
 * of stages[K-1].h; only the arrays asked for cross the bus.  Returns when every output is in place. */
int gpt_pullback_chain(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y, const double* x0, int64_t M,
                       double rtol, int max_passes, double std_offset, double* x, double* vel, double* f, int* status, double* var_dyn,
                       double* vel_var_map, double* vel_var_dyn, double* stage_x, double* stage_z, double* stage_A, double* stage_Jvar,
                       double* stage_map_var, int* stage_status, int* stage_passes, double* stage_residual, double* stage_det);

/* (new) Whole paths of the transported policy: the mean policy of gpt_pullback_chain integrated from M starts with n_steps = T
 * explicit Euler steps of size dt, the loop over the steps on the device (the reference's plot_traj_evolution is 1000 steps of
 * pos += vel on the host).  stages, K, h_dyn, rtol, max_passes as gpt_pullback_chain, with K = 0 (stages may then be NULL) allowed:
 * the dynamics rolls out itself.  Inputs: y0 (M,D) the starts; x0 (M,D) guesses of the SOURCE-space preimages of the starts, or
 * NULL; dt finite and not zero (negative: backwards).  Per trajectory m, for t = 0 .. T-1:
 *   (x_t, vel_t, status_t) = exactly what gpt_pullback_chain returns as x, vel, status for the single point y_t, with the guess
 *                x_{t-1} (at t = 0: x0[m], or none).  K = 0: x_t = y_t, vel_t = the mean of h_dyn at y_t, status_t = CONVERGED.
 *   y_{t+1} = y_t + (dt vel_t), the product and the sum rounded separately (no fused multiply-add: y + dt * vel in C or numpy).
 *   The trajectory ENDS at the first t where status_t is not GPT_INV_CONVERGED or y_{t+1} is not finite: x_t, vel_t and status_t
 *   are still recorded, y_{t+1} is not.
 * Outputs, trajectory-major:
 *   path (M,T+1,D)    row 0 = y0, row t+1 = y_{t+1}; NaN after a trajectory's end
 *   vel, x (M,T,D)    either may be NULL; NaN after the end
 *   steps_done (M, int)  the steps whose y_{t+1} was recorded (T: the trajectory never ended)
 *   status (M, int)   the GPT_INV_* of the last step evaluated; CONVERGED when T = 0
 * One wave per trajectory (k_rollout, around the per-point body of k_chain_velocity); a launch advances every live trajectory by at
 * most 64 steps (the environment's GPT_ROLLOUT_STEPS_PER_LAUNCH, read per call, overrides), the launches of a call are enqueued
 * back to back with no host read in between, and a trajectory that has ended costs a later launch one wave that returns at once.
 * A trajectory's values do not depend on M, on the other trajectories, on their order or on where the launches are cut, bit for bit.
 * Refusals: gpt_pullback_chain's (K = 0 .. GPT_CHAIN_MAX here; for K = 0 what it refuses of a dynamics model), and GPT_E_ARG for
 * n_steps < 0; dt zero, NaN or infinite; M (n_steps + 1) >= 2^31; a NULL among y0, path, steps_done, status.  M = 0 does nothing;
 * n_steps = 0 writes path = y0.
 * Device memory.  Asynchronous: enqueued on the stream of stages[K-1].h (K = 0: of h_dyn), which first waits for what the other
 * handles' streams hold so far; they go on after the last launch.  No host synchronisation.  Scratch, staging and events belong to
 * stages[K-1].h (K = 0: h_dyn), grow-only; device memory per call: M D doubles (the carried x) when the call takes more than one
 * launch, else none.  Every model is left as it was. */
int gpt_rollout_policy_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0_dev, const double* x0_dev, int64_t M,
                           int64_t n_steps, double dt, double rtol, int max_passes, double* path_dev, double* vel_dev, double* x_dev,
                           int* steps_done_dev, int* status_dev);
/* (new) The same with every data pointer in host memory; also GPT_E_ARG for NaN / infinity in y0, x0, an affine part or rtol.  The
 * trajectories are streamed through the device in chunks of max(1, 131072 / (n_steps + 1)) through two staging sets of the owning
 * handle, so a chunk's images hold about 131072 path rows whatever n_steps is: two sets of at most
 * chunk ((3 n_steps + 1) D + 2 D) doubles and 2 chunk ints, less for what was not asked for; only the arrays asked for cross the
 * bus.  Returns when every output is in place. */
int gpt_rollout_policy(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0, int64_t M,
                       int64_t n_steps, double dt, double rtol, int max_passes, double* path, double* vel, double* x, int* steps_done,
                       int* status);

/* (new) Whole paths of the VARIANCE-STABILISED policy: gpt_rollout_policy with the stabiliser of the reference's plot_traj_evolution
 * (pos += mean - std * grad_var / |grad_var|) inside every step, still one call.  Arguments, end rule, NaN filling, steps_done,
 * status, the guesses, negative dt, launches and chunks as gpt_rollout_policy; in addition gain (finite, >= 0) and std_offset (the
 * caller passes sqrt(noise_level), the reference's predict(return_std) quirk, as gpt_pullback_chain's).  Per trajectory and step,
 * x_t the source-space preimage of y_t (K = 0: x_t = y_t), W = L^-1 the inverse factor of the dynamics, c its prior variance:
 *   f_t     = the mean of h_dyn at x_t
 *   var_t   = max(0, c + noise - |W k*(x_t)|^2),   g_t,d = -2 (W d_d k*(x_t)) . (W k*(x_t))   (gpt_predict_all's var and dvar)
 *   s_t     = sqrt(var_t) - std_offset
 *   ghat_t  = g_t / |g_t|, the norm taken after scaling by max_d |g_t,d| (a tiny gradient does not underflow to a zero norm);
 *             ghat_t = 0 where every g_t,d is exactly 0 (k* has underflowed far from the data; the reference divides 0 by 0 there)
 *   fs_t,d  = f_t,d - ((gain s_t) ghat_t,d), each product and the difference rounded on its own
 *   vel_t   = fs_t pushed through the maps exactly as gpt_pullback_chain pushes f (K = 0: vel_t = fs_t)
 *   y_{t+1} = y_t + (dt vel_t)
 * A g that is not finite makes y_{t+1} not finite, which ends the trajectory.  For K >= 1 the target-space path is, to first order
 * in dt, the image of the stabilised source-space path: the variance descended is the dynamics' own at the preimage, not that of a
 * GP refitted on the moved demonstration.  gain = 0 gives the path, vel, x, steps_done and status of gpt_rollout_policy, bit for bit.
 * Further outputs, each may be NULL, NaN after a trajectory's end: f (M,T,D), var (M,T), dvar (M,T,D) = g.
 * One workgroup of four waves owns four trajectories and shares the product with W on the matrix cores (k_rollout_stab); a launch
 * advances every live trajectory by at most 32 steps (GPT_ROLLOUT_STEPS_PER_LAUNCH overrides).  A trajectory's values do not depend
 * on M, on the other trajectories, on their order or on where the launches are cut, bit for bit.
 * Refusals beyond gpt_rollout_policy's, GPT_E_ARG: a dynamics of more than 1024 training points (the kernel columns of a step stay
 * in LDS); a Matern 1/2 dynamics, or a Matern 3/2 / 5/2 one without gpt_set_matern_derivatives; gain negative, NaN or infinite;
 * std_offset NaN or infinite.  (Multi-task and fp32 models are refused as by gpt_rollout_policy.)
 * Device memory, asynchronous, streams and resources as gpt_rollout_policy_dev (the two calls share them). */
int gpt_rollout_stabilised_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0_dev, const double* x0_dev, int64_t M,
                               int64_t n_steps, double dt, double rtol, int max_passes, double gain, double std_offset, double* path_dev,
                               double* vel_dev, double* x_dev, double* f_dev, double* var_dev, double* dvar_dev, int* steps_done_dev,
                               int* status_dev);
/* (new) The same with every data pointer in host memory, checked and chunked as gpt_rollout_policy. */
int gpt_rollout_stabilised(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0, int64_t M,
                           int64_t n_steps, double dt, double rtol, int max_passes, double gain, double std_offset, double* path,
                           double* vel, double* x, double* f, double* var, double* dvar, int* steps_done, int* status);

/* (new) Whole paths of FUNCTIONS DRAWN FROM THE DYNAMICS POSTERIOR: gpt_rollout_policy with, in place of the dynamics mean, one
 * function drawn from the posterior of h_dyn per path, still one call.  The value drawn at step t is conditioned on what the same
 * function was drawn to be at the path's own earlier points, so a path that revisits a region meets the same function there.  Only
 * the dynamics is sampled; the maps act through their means.  Arguments, end rule, NaN filling, steps_done, the guesses, negative
 * dt, launches and chunks as gpt_rollout_policy (M: the number of paths); in addition normals (M,T,D), standard normal numbers of
 * the caller (the device generates none: given normals the call is a deterministic function), and nugget (finite, >= 0), added to
 * the diagonal of a path's covariance: the model's noise level draws noisy values, the convention of gpt_predict_cov; a small
 * positive number draws the latent function.  Per path and step, x_t the source-space preimage of y_t (K = 0: x_t = y_t),
 * W = L^-1 the inverse factor of the dynamics, c its prior variance, k its kernel without noise:
 *   f_t     = the mean of h_dyn at x_t
 *   u_t     = W k*(x_t),   pvar_t = (c + nugget) - u_t . u_t
 *   c_ts    = k(x_t, x_s) - u_t . u_s                                  s < t
 *   g_ts    = (c_ts - sum_{r<s} g_tr g_sr) / g_ss, s ascending         row t of the lower factor G of the path's covariance
 *   cvar_t  = pvar_t - sum_{s<t} g_ts^2                                the variance of the draw given the earlier ones
 *   cvar_t NaN or <= 1024 * 2^-52 * (c + nugget): the path ENDS at step t with status GPT_ROLLOUT_DEGENERATE (x_t, f_t, pvar_t and
 *             cvar_t are recorded, vel_t is NaN); mathematically cvar_t >= nugget, so a nugget above that floor never ends a path
 *   g_tt    = sqrt(cvar_t)
 *   fs_t,d  = f_t,d + sum_{r<=t} g_tr normals[r,d], r ascending, each product and sum rounded on its own
 *   vel_t   = fs_t pushed through the maps exactly as gpt_pullback_chain pushes f (K = 0: vel_t = fs_t)
 *   y_{t+1} = y_t + (dt vel_t)
 * With all normals zero: the path, vel, x, steps_done and status of gpt_rollout_policy, bit for bit but for the sign of a zero.
 * status (M, int): the GPT_INV_* of gpt_rollout_policy, or GPT_ROLLOUT_DEGENERATE.  A step whose inverse does not converge ends the
 * path with that GPT_INV_* and its vel_t recorded, as in gpt_rollout_policy, with one exception: where the pivot of that same step is
 * also degenerate there is no draw, and vel_t is NaN.  Further outputs, each may be NULL, NaN after a
 * path's end: f (M,T,D), pvar (M,T), cvar (M,T), chol (M,T,T) = G, the lower triangle with zeros above it (the row of a degenerate
 * step is NaN).
 * One workgroup of four waves owns sixteen paths and shares the product with W on the matrix cores (k_rollout_sampled); a launch
 * advances every live path by at most GPT_ROLLOUT_STEPS_PER_LAUNCH steps (default: gpt_rollout_sampled.h).  A path's values do not
 * depend on M, on the other paths, on their order or on where the launches or the chunks are cut, bit for bit.
 * Refusals beyond gpt_rollout_policy's, GPT_E_ARG: a dynamics of more than 1024 training points; n_steps above
 * GPT_ROLLOUT_SAMPLED_MAX_T; nugget negative, NaN or infinite; normals NULL with M > 0 and n_steps > 0; a call whose scratch (u
 * of every step, 128 ceil(M / 16) n_steps ceil(N / 64) 64 bytes, the factor, 8 M n_steps (n_steps + 8) bytes) exceeds 80 % of the device's free
 * memory.  (Multi-task and fp32 models are refused as by gpt_rollout_policy; any of the four kernels is taken.)
 * Device memory, asynchronous, streams and resources as gpt_rollout_policy_dev (the calls share them). */
#define GPT_ROLLOUT_DEGENERATE 4
#define GPT_ROLLOUT_SAMPLED_MAX_T 256
int gpt_rollout_sampled_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0_dev, const double* x0_dev,
                            const double* normals_dev, int64_t M, int64_t n_steps, double dt, double rtol, int max_passes, double nugget,
                            double* path_dev, double* vel_dev, double* x_dev, double* f_dev, double* pvar_dev, double* cvar_dev,
                            double* chol_dev, int* steps_done_dev, int* status_dev);
/* (new) The same with every data pointer in host memory, checked and chunked as gpt_rollout_policy; also GPT_E_ARG for NaN or infinity
 * in normals.  A chunk is further held to the paths whose scratch stays below 1 GiB (at least sixteen;
 * GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES overrides the budget). */
int gpt_rollout_sampled(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0, const double* normals,
                        int64_t M, int64_t n_steps, double dt, double rtol, int max_passes, double nugget, double* path, double* vel,
                        double* x, double* f, double* pvar, double* cvar, double* chol, int* steps_done, int* status);

/* (new) Whole paths of WHOLE FUNCTIONS DRAWN FROM THE DYNAMICS POSTERIOR by pathwise conditioning (Matheron's rule, the prior as a
 * sum of random Fourier features): gpt_rollout_policy with, in place of the dynamics mean, one of S deterministic functions
 *   F_s(x) = sum_n k(x, X_n) V_s[n, :]  +  sum_j ( a_sj cos(omega_j . x) + b_sj sin(omega_j . x) ),
 * k and X the kernel (without noise) and the training points of h_dyn.  The caller draws omega and the amplitudes and solves for
 * V_s = (K + sigma^2 I)^-1 (Y - prior_s(X) - sigma eps_s) once per function (gpt_apply_inverse); the device generates no random
 * number, so the call is a deterministic function of its arguments.  Unlike gpt_rollout_sampled, a function here exists everywhere:
 * paths of one function from different starts see the same field, a step costs O(N + J) whatever t is, and neither N nor n_steps
 * has a limit of its own.  The approximation is in the prior only (its covariance error falls as 1 / sqrt(J)); the update against
 * the data is exact.  Only the dynamics is sampled; the maps act through their means.
 * Arguments, end rule, NaN filling, steps_done, status, the guesses, negative dt, launches and chunks as gpt_rollout_policy (M: the
 * number of paths); in addition
 *   func (M, int)      path p follows function func[p], 0 .. S - 1
 *   S                  the number of functions, >= 1
 *   weights            the V_s.  Host entry: (S,N,D).  Device entry: (S,NP,4), one image per function in the layout of the model's
 *                      alpha rows: row n = (V_s[n, 0 .. D-1], zeros), zero rows from N up to NP = N rounded up to a multiple of 512
 *   J                  the number of frequencies, 0 .. GPT_PATHWISE_MAX_FREQ
 *   omega (J,D), amp (S,J,2,D)   the frequencies; per function and frequency the D cosine amplitudes, then the D sine amplitudes
 * Per path and step, s = func[p], x_t the source-space preimage of y_t (K = 0: x_t = y_t):
 *   u_t     = sum_n k(x_t, X_n) V_s[n, :], the arithmetic of the dynamics mean on the function's weights
 *   theta_j = sum_d omega_jd x_t,d, d ascending;   p_t = sum_j a_sj cos(theta_j) + b_sj sin(theta_j), one sincos per j
 *   fs_t    = u_t + p_t
 *   vel_t   = fs_t pushed through the maps exactly as gpt_pullback_chain pushes f (K = 0: vel_t = fs_t)
 *   y_{t+1} = y_t + (dt vel_t)
 * With J = 0 and every V_s the model's alpha: the path, vel, x, steps_done and status of gpt_rollout_policy, bit for bit but for
 * the sign of a zero.  Further output, may be NULL, NaN after a path's end: f (M,T,D) = fs.
 * One wave per path (k_rollout_pathwise: k_rollout's step with the feature sum added); a launch advances every live path by at
 * most 128 steps (GPT_ROLLOUT_STEPS_PER_LAUNCH overrides; gpt_rollout_pathwise.h).  A path's values do not depend on M, on S, on the other paths or functions,
 * on their order or on where the launches or the chunks are cut, bit for bit.
 * Refusals beyond gpt_rollout_policy's, GPT_E_ARG: S < 1; J < 0 or J > GPT_PATHWISE_MAX_FREQ; func or weights NULL with M > 0; omega
 * or amp NULL with M > 0 and J > 0.  (Multi-task and fp32 models are refused as by gpt_rollout_policy; any of the four kernels is
 * taken as the dynamics.)  The device entry does not read func on the host: a path whose entry is
 * outside 0 .. S - 1 ends before its first step with steps_done = 0, status = GPT_ROLLOUT_NO_FUNCTION and NaN in every row of its
 * outputs, row 0 of path included; nothing is read out of bounds.
 * Device memory, asynchronous, streams and resources as gpt_rollout_policy_dev (the calls share them). */
#define GPT_PATHWISE_MAX_FREQ 8192
#define GPT_ROLLOUT_NO_FUNCTION (-1)
int gpt_rollout_pathwise_dev(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0_dev, const double* x0_dev,
                             const int* func_dev, int64_t M, int64_t n_steps, double dt, double rtol, int max_passes, int64_t S,
                             const double* weights4_dev, int64_t J, const double* omega_dev, const double* amp_dev, double* path_dev,
                             double* vel_dev, double* x_dev, double* f_dev, int* steps_done_dev, int* status_dev);
/* (new) The same with every data pointer in host memory, checked and chunked as gpt_rollout_policy; weights (S,N,D) are packed into
 * the images here.  Also GPT_E_ARG for a func entry outside 0 .. S - 1 and for NaN or infinity in weights, omega or amp.  The
 * images, omega and amp are uploaded once per call into the scratch of the owning handle (S NP 4 + J D + 2 S J D doubles,
 * grow-only); the paths are chunked as gpt_rollout_policy's (GPT_ROLLOUT_PATHWISE_CHUNK in the environment: at most so many paths
 * per chunk). */
int gpt_rollout_pathwise(const gpt_chain_stage* stages, int K, gpt_handle* h_dyn, const double* y0, const double* x0, const int* func,
                         int64_t M, int64_t n_steps, double dt, double rtol, int max_passes, int64_t S, const double* weights, int64_t J,
                         const double* omega, const double* amp, double* path, double* vel, double* x, double* f, int* steps_done,
                         int* status);

/* predict(return_cov=True) — replaces sklearn/_gpr.py:458-470: mean (M,O) (may be NULL) and the joint
 * posterior covariance cov (M,M) = k(Xq,Xq) + noise_level*I - V^T V, V = L^-1 K*^T (identical for every
 * output; the caller tiles it).  Small-M path used by GaussianProcess.samples (gaussian_process.py:57-60);
 * M <= 16384; needs the handle that ran gpt_fit.  Host memory. */
int gpt_predict_cov(gpt_handle* h, const double* Xq, int64_t M, double* mean, double* cov);

/* Parity-test export of sklearn's fitted attributes: L (N,N) lower triangular (zeros above),
 * alpha (N,O).  Either may be NULL.  Host memory. */
int gpt_export(gpt_handle* h, double* L, double* alpha);
/* W = L^-1 (N,N) lower triangular, host memory (tests only). */
int gpt_export_inverse_factor(gpt_handle* h, double* W);
/* (new) out = (K + sigma^2 I)^-1 R for C caller-supplied columns: W^T (W R) with the inverse factor of the fitted model, through the
 * launches that compute alpha in gpt_fit (R = Y gives the alpha of gpt_export, bit for bit).  R, out: (N,C) row-major, host memory,
 * may be the same array.  The columns go through the device four per pass, the last pass padded with zero columns; a column's
 * result does not depend on the other columns of the call, bit for bit.  Rows of R beyond the model's N do not exist: R has exactly
 * the N rows of the training set, in its order.  C = 0 does nothing.
 * Refusals: GPT_E_STATE without a fitted model; GPT_E_ARG for an fp32 model, a multi-task gpt_fit_svgp model, a handle that did not
 * run gpt_fit for this model (a gpt_factor_copy replica, a committed blob: they hold no W), C < 0, R or out NULL with C > 0.
 * Synchronous on the handle's stream: returns when out is in place.  Device memory: 2 NP 4 doubles of the handle's covariance
 * scratch (grow-only); the model and the factors are left as they were. */
int gpt_apply_inverse(gpt_handle* h, const double* R, int64_t C, double* out);

/* Log-marginal likelihood of the fitted theta (sklearn/_gpr.py:598-606): sum over outputs of
 * -0.5 y^T alpha - sum(log diag L) - N/2 log(2 pi). */
int gpt_lml(gpt_handle* h, double* lml);
/* The same value plus its gradient with respect to theta = log [constant_value, length_scale (n_ls
 * entries), noise_level] — what sklearn's optimizer consumes (sklearn/_gpr.py:625-648: 0.5 * trace((alpha
 * alpha^T - K^-1) dK/dtheta) summed over outputs).  grad has 2 + n_ls entries.  Overwrites the Cholesky
 * factor held for gpt_export (a later gpt_fit restores it). */
int gpt_lml_gradient(gpt_handle* h, double* lml, double* grad);

/* One evaluation of the optimizer's objective in one call: what gpt_fit_kernel + gpt_lml_gradient return for these
 * hyper-parameters, without building the prediction-side model (no packed inverse factor, no alpha in the model's
 * layout) — the inner loop of GaussianProcess.fit with optimizer='fmin_l_bfgs_b' (sklearn/_gpr.py:296-338: every
 * L-BFGS-B step evaluates the LML and its gradient).  Afterwards the handle holds NO model (predict needs a gpt_fit). */
int gpt_lml_objective(gpt_handle* h, const double* X, const double* Y, int64_t N, int D, int O,
                      const double* length_scale, int n_ls, double constant_value, double noise_level,
                      double alpha_jitter, int kernel_type, double* lml, double* grad);

/* Multi-GPU hand-off of a fitted model (fit on rank 0, predict shards everywhere).  The model
 * is one contiguous device blob {header, scaled X, alpha, packed L^-1}:
 *   rank 0   : gpt_fit(...); gpt_factor_blob(h, &ptr, &bytes)
 *   others   : gpt_factor_alloc(h, N, D, O, &ptr, &bytes)        (same N, D, O)
 *   all      : broadcast `bytes` bytes at `ptr` (RCCL, e.g. torch.distributed.broadcast)
 *   others   : gpt_factor_commit(h)                                (parses the header)           */
int gpt_factor_blob(gpt_handle* h, void** dev_ptr, size_t* bytes);
int gpt_factor_alloc(gpt_handle* h, int64_t N, int D, int O, void** dev_ptr, size_t* bytes);
/* The same for any model: n_tasks = 1 and GPT_F64 for gpt_fit*, (T, dtype) for gpt_fit_svgp — see gpt_model_info. */
int gpt_factor_alloc_model(gpt_handle* h, int64_t N, int D, int O, int n_tasks, int dtype, void** dev_ptr, size_t* bytes);
int gpt_factor_commit(gpt_handle* h);
/* The same hand-off inside ONE process (a handle per GPU, SURVEY section 8b's n_devices): copies src's fitted model
 * blob to dst's device (hipMemcpyPeerAsync over xGMI; a device-to-device copy when both handles sit on one GPU) and
 * commits it.  Afterwards dst predicts exactly what src predicts.  What GaussianProcess(devices=[...]) calls after fit so
 * that predict / derivative (gaussian_process.py:46-55, 63-102) can shard their rows over the GPUs behind the same class
 * (transportation/gaussian_process_transportation.py:19-26 never sees the devices).  dst's fit-side state (L, W) is not
 * copied: export / return_cov / LML stay with the handle that ran the fit. */
int gpt_factor_copy(gpt_handle* dst, gpt_handle* src);

/* Model geometry of a fitted / committed handle. */
int gpt_info(gpt_handle* h, int64_t* N, int* D, int* O, int64_t* N_padded);

/* Stacked tasks (1 unless fitted by gpt_fit_svgp) and element type (GPT_F64 / GPT_F32) of the model. */
int gpt_model_info(gpt_handle* h, int* n_tasks, int* dtype);

/* Per-phase device times of the last gpt_fit in milliseconds (hipEvent):
 * [0] total [1] gram [2] cholesky [3] triangular inverse [4] alpha [5] pack.  n <= 6. */
int gpt_fit_timings(gpt_handle* h, double* ms_out, int n);

/* Per-kernel device times of the last gpt_predict_all_dev call.  With profiling enabled the call
 * records hipEvents around each kernel on the handle's stream (no host synchronisation);
 * gpt_predict_timings waits for them and returns ms_out[0] = mean+Jacobian contraction kernel,
 * ms_out[1] = variance (MFMA) kernel; 0 for a kernel that was not launched. */
int gpt_set_profiling(gpt_handle* h, int enable);
int gpt_predict_timings(gpt_handle* h, double* ms_out);
/* Which kernel the last variance launch of this handle took: 0 the fp64 kernel, 1 the residue (int8) kernel, -1 no launch yet.
 * The int8 path takes k*-alone launches of fp64 single-task models with D <= 3; GPT_VAR_INT8 = 0 / 1 in the environment forces
 * it off / on (read per call). */
int gpt_debug_var_path(gpt_handle* h);

/* Test hook (host only, no GPU): the work decomposition of the variance kernel for a launch of n_columns kernel
 * columns over n_iblocks 512-row blocks x n_tasks tasks on n_workgroups workgroups (csrc/gpt_plan.h).
 * order: -1 automatic, 0 block-major, 1 sweep-major.  counts[12] = {items, cut sweeps, slab slots, partial-product
 * slots, column blocks, blocks in whole rounds, tail (block, task) pairs, order used, cohort plan used (0 / 1), its first whole
 * i-block s, tiles f of sweep s - 1 taken with the long sweeps, diagonal tiles divisible in this list (0 / 1)}; item k ranges
 * count quarter tiles; a cut sweep owns 8 consecutive slab slots from splits[.][2]; the arrays may be NULL (first
 * call) or hold item_begin[n_workgroups + 1], items[counts[0]][8], fin[counts[6]][2], splits[counts[1]][3]. */
int gpt_debug_var_plan(int64_t n_columns, int n_iblocks, int n_tasks, int n_workgroups, int order, int64_t* counts,
                       int* item_begin, int* items, int* fin, int* splits);

/* Test hook (host only, no GPU): the plan of the factor + inverse for a padded size (csrc/gpt_fit_plan.h).
 * form: 0 one leaf, 1 split with the second half's chain beside the first half's inverse, 2 left-looking panels with look-ahead,
 * < 0: environment / by size; panel (form 2) and streams (1 = CU-masked side and chain streams, 0 = the serial order) < 0:
 * environment or defaults.  counts[6] = {ops, arena doubles, form, events, doubles the fit workspace allocates (>= arena),
 * eighths of the CUs given to the side stream}; ops (may be NULL) receives counts[0] rows of 18: kind, stream, off, n1, n2, k0,
 * kw, row_end, grp, r0, r0_size, r1, r1_size, wait0, wait1, wait2, record, 0 (regions in doubles inside the arena; events by id,
 * -1 = none; FitOpKind and the streams in gpt_fit_plan.h). */
int gpt_debug_fit_plan(int n_padded, int form, int panel, int streams, int64_t* counts, int64_t* ops);

/* Test hook (needs a GPU): one call of the library's fp64 MFMA GEMM (k_gemm behind launch_dgemm, csrc/gpt_common.h) on host
 * operands.  C (M x N, ldc) = alpha op(A) op(B): at -> op(A) = A^T with A stored (K x M, lda); bt -> op(B) = B^T with B stored
 * (N x K, ldb); not both.  lower_only (M == N): only the block lower triangle of C is computed (tiles above the diagonal and
 * the upper wave quadrants of diagonal tiles are not written).  The WHOLE image of C (M x ldc doubles) goes to the device and
 * comes back, so that a caller can pre-fill it and look for stray writes; A and B are read as (rows x ld) images too.
 * tile_edge receives the tile edge the launcher chose for this product (32, 64 or 128).  GPT_E_ARG for what launch_dgemm's
 * contract excludes: M, N, K not multiples of 64, at && bt, lower_only with M != N, a leading dimension smaller than its row,
 * odd or above 2^26. */
int gpt_debug_dgemm(int device, int at, int bt, int M, int N, int K, double alpha, const double* A, int64_t lda,
                    const double* B, int64_t ldb, double* C, int64_t ldc, int lower_only, int* tile_edge);

/* Test hook (needs a GPU): W (n x n, dense, row-major, host memory) replaces the inverse factor of a committed single-task model
 * on the handle that ran its own gpt_fit (fp64 or fp32 model), so that the variance kernels can be given operands whose answer
 * is known exactly.  W goes to the fit workspace, is packed into the model's image with the model's element type, and the residue
 * (int8) planes are rebuilt under the rule of gpt_factor_commit; the upper triangle of W is ignored, as the fit's own packing
 * ignores it.  gpt_export_inverse_factor returns W afterwards - its upper triangle as the caller passed it, which no kernel reads
 * and the next gpt_fit overwrites: compare lower triangles; gpt_export(L), gpt_lml and gpt_lml_gradient refuse until the next
 * gpt_fit (L is the factor of another matrix).  GPT_E_ARG: NULL argument, n != N; GPT_E_STATE: no committed model, a multi-task
 * model, a replica (gpt_factor_commit / gpt_factor_copy) that holds no factor of its own. */
int gpt_debug_set_inverse_factor(gpt_handle* h, const double* W, int64_t n);

/* Test hook (needs a GPU): the same for task `task` of a multi-task model, on the handle that ran its gpt_fit_svgp.  W takes the
 * place of the task's inverse factor in the packed image, multiplied by the task's outputscale as the fit's own packing does;
 * the other tasks' factors and every alpha stay.  (A multi-task handle keeps no dense factor: nothing is exported afterwards,
 * as nothing was before.)  A single-task model: task must be 0, and the call is gpt_debug_set_inverse_factor.  GPT_E_ARG: NULL
 * argument, task outside 0 .. n_tasks - 1, n != N; GPT_E_STATE: no committed model, a replica without the fit's workspace. */
int gpt_debug_set_task_inverse_factor(gpt_handle* h, int task, const double* W, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* GPT_HIP_H */
