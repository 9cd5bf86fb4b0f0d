/*
 * tensor_regression_hip.h — C ABI of the MI355X (gfx950) CP tensor-regression hot path.
 *
 * This is the drop-in boundary for the reference's forward/gradient loop
 * (kimerein/tensor_regression).  The reference has no FFI layer of its own: its hot path
 * is the pure-Python/torch sequence
 *
 *     lin_model / model  ->  loss_fn + lambda_L2 * L2_penalty  ->  loss.backward()
 *                        ->  optimizer.step()  ->  loss_running.append(loss.item())
 *
 * in standard_tensor_regression.py:458-470 (CP_linear_regression.fit_Adam) and
 * multinomial_tensor_regression.py:453-465 (CP_logistic_regression.fit_Adam).  Each entry
 * point below replaces one contiguous piece of that sequence; the Python package
 * `tensor_regression_amd` binds them with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - Every pointer argument is DEVICE memory on the plan's device unless stated otherwise;
 *     the library never frees memory it did not allocate.
 *   - fp32 (the reference's multinomial and spectral classes are fp32-only,
 *     multinomial_tensor_regression.py:255; the standard class defaults to fp32, :206), plus a
 *     float64 linear model through the *_f64 entry points (CP_linear_regression(dtype=
 *     torch.float64), standard_tensor_regression.py:206).
 *   - X is sample-major and C-contiguous: X[n, i_1, ..., i_K], i.e. an (N x P) row-major
 *     matrix with P = prod(dims).
 *   - Parameter arena: the Kruskal factor list `Bcp` packed back to back in the reference's
 *     list order, each factor (I_f x R) row-major, followed by the scalar bias for the
 *     linear model: [A_1 | A_2 | ... | A_F | (bias)].  tr_plan_factor_offset() gives the
 *     offsets; tr_plan_num_params() the total.
 *   - Gradient arena: same layout as the parameter arena plus TWO trailing slots: the data
 *     loss, then the device status (0.0 = the pass succeeded; nonzero = a kernel of the pass
 *     failed, see tr_plan_status), i.e. tr_plan_num_grads() = tr_plan_num_params() + 2.
 *     Both slots survive the cross-shard sum meaningfully.  Data-term gradients
 *     are already normalised by the GLOBAL sample count (linear) or class-weight total
 *     (multinomial), so the element-wise sum of the arenas of disjoint sample shards is the
 *     full-data gradient — one all-reduce(sum) per iteration is the only exchange.
 *   - `stream` is a hipStream_t passed as void*; all calls are asynchronous on it.
 *   - Return value: 0 on success, < 0 invalid argument (TR_E_*), > 0 a hipError_t.
 *     tr_last_error() returns a thread-local message for the last failure.
 *   - `stop_flag` (int32 device scalar, may be NULL): when non-zero every kernel of the
 *     iteration returns immediately.  tr_adam_step sets it when the reference's plateau
 *     test fires (standard_tensor_regression.py:467-470), which lets the host enqueue many
 *     iterations without a per-iteration host synchronisation.
 */
#ifndef TENSOR_REGRESSION_HIP_H
#define TENSOR_REGRESSION_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TR_ABI_VERSION 9

#define TR_MODEL_LINEAR 0      /* CP_linear_regression: y_hat = <X, [[w; Phi]]> + bias, MSE */
#define TR_MODEL_MULTINOMIAL 1 /* CP_logistic_regression: softmax(<X, [[w; Phi]]>), CE(weight) */
#define TR_MODEL_SPECTRAL 2    /* spectral CP_linear_regression: lin_model + stepwise_spectral_model, MSE */

#define TR_MODEL_CONV_SPECTRAL 3 /* convolutional spectral CP_linear_regression on the untiled (T, D) series */

#define TR_MAX_FACTORS 8

/* *stop_flag written by tr_adam_step when the gradient arena's status slot is set: the step was
 * NOT applied, parameters and Adam state are those after iteration `iter - 1`.
 * Value = TR_STOP_DEVICE_ERROR - iter (plateau stops are > 0, spectral NaN stops > -2^30). */
#define TR_STOP_DEVICE_ERROR (-(1 << 30))

#define TR_E_ARG (-1)      /* invalid argument (shape/size/pointer) */
#define TR_E_UNSUPPORTED (-2)
#define TR_E_NOMEM (-3)

typedef struct tr_plan tr_plan;

/* Library ABI version (TR_ABI_VERSION). */
int tr_abi_version(void);

/* SHA-256 (hex) of the sources the library was compiled from (the .hip and .h files of csrc,
 * in byte order of their names, then this header); the Python loader refuses a library whose id
 * does not match the sources next to it. */
const char* tr_build_id(void);

/* Thread-local message describing the most recent failure ("" if none). */
const char* tr_last_error(void);

/*
 * Create a plan for one model shape on `device` and allocate its workspace.
 * Replaces the shape bookkeeping of CP_linear_regression.__init__
 * (standard_tensor_regression.py:204-303) / CP_logistic_regression.__init__
 * (multinomial_tensor_regression.py:212-286).
 *   model          TR_MODEL_LINEAR or TR_MODEL_MULTINOMIAL
 *   n_feature_modes K = X.ndim - 1 (1 .. TR_MAX_FACTORS-1)
 *   feature_dims   host array of K dims (I_1 .. I_K)
 *   n_classes      multinomial: C (the extra factor has C rows); linear: ignored (use 1)
 *   rank           R (1 .. 1024)
 *   max_rows       largest sample count later passed to tr_loss_grad (sizes the workspace)
 *   non_negative   host array, one flag per factor (K linear / K+1 multinomial): softplus
 *                  is applied to flagged factors (non_neg_fn, standard…py:53-85)
 *   softplus_beta / softplus_threshold   torch.nn.functional.softplus kwargs
 */
int tr_plan_create(tr_plan** out, int device, int model, int n_feature_modes,
                   const int64_t* feature_dims, int n_classes, int rank, int64_t max_rows,
                   const int32_t* non_negative, float softplus_beta, float softplus_threshold);

int tr_plan_destroy(tr_plan* plan);

int64_t tr_plan_num_params(const tr_plan* plan); /* factors (+ bias) */
int64_t tr_plan_num_grads(const tr_plan* plan);  /* num_params + 2 (data-loss + status slots) */
int64_t tr_plan_factor_offset(const tr_plan* plan, int factor);
int64_t tr_plan_workspace_bytes(const tr_plan* plan);
/* Human-readable description of the kernel strategy the next call on this plan runs (host string):
 * written at creation and rewritten whenever tr_plan_set_x_stride re-chooses the strategy. */
const char* tr_plan_describe(const tr_plan* plan);

/*
 * Row stride of X for the following tr_forward / tr_loss_grad / tr_spectral_latents calls:
 * sample n starts at X + n*stride floats and its P floats are contiguous (stride 0 = P, the
 * dense default).  A stride < P expresses the reference's windowed samples
 * (util.py:67-114, WindowedDataset: sample n = rows [n + w0, n + w1) of an untiled (T, F...)
 * series) without materialising them: stride = F, P = window * F.  The vector (16-byte) kernel
 * paths need stride % 4 == 0 and a 16-byte aligned X; otherwise the plan switches to its scalar
 * paths, and a misaligned X on a vector plan is rejected with TR_E_ARG.  tr_plan_describe follows
 * the re-chosen strategy; stride 0 restores the creation-time strategy and its text.
 */
int tr_plan_set_x_stride(tr_plan* plan, int64_t stride);

/*
 * Range statistics of a sample-major X (n_rows rows of P floats at row stride xld; xld = 0: P;
 * rows may overlap): workgroup b of nblocks (1..1024) writes out[b] = max |x|,
 * out[nblocks + b] = the smallest mean x^2 of a row that is not all zero (+inf if none) and
 * out[2 nblocks + b] = min x (doubles) over its rows, asynchronously on `stream`; the caller
 * reduces the 3 * nblocks values (max, min, min).  One streaming read of X.  No reference
 * counterpart: it guards the split kernels' number formats (tr_plan_set_x_range).
 */
int tr_x_range(const float* X, int64_t n_rows, int64_t P, int64_t xld, double* out, int nblocks, void* stream);

/*
 * X's range for the plan's next tr_loss_grad calls (max |x|, the smallest mean x^2 of a nonzero
 * sample, and min x, e.g. from tr_x_range).
 *  - The multinomial factored pass in its bf16-split form represents X as a bf16 piece plus an f16
 *    residual, within 2^-20 |x| + 2^-25 of x — per sample normwise 2^-20 + 2^-25 / rms(sample) —
 *    while every nonzero sample's rms >= 2^-5 and max |x| < 2^23; outside that range (or for a
 *    non-finite value) the plan runs its exact form (three bf16 pieces, x represented exactly,
 *    ~15-20 % slower).
 *  - The spectral column-slice kernel in its split form takes X in two bf16 pieces; on signed X
 *    (min x < 0: the forward T = X Phi0 cancels) the plan runs its signed form (the forward's X in
 *    three pieces and per-sample gradient accumulators, ~13 % slower).
 * Re-set after every tr_plan_set_x_stride call (which resets the plan to its default form).
 * Plans of other kernels ignore it.  The Python layer calls both once per X (Plan._x_form).
 */
int tr_plan_set_x_range(tr_plan* plan, double max_abs, double min_row_mean_sq, double min_x);

/*
 * The multinomial factored pass's shape decision for two-mode samples (I, J), rank R, C classes,
 * without a device (ABI 8): out[0] = 1 if the two-workgroups-per-CU family (k_mnl_duo / k_mnl_bsp)
 * takes the shape, [1] = 1 for its bf16-split body (0: the rank-block body), [2] waves per
 * workgroup, [3] workgroups per CU, [4] ring slots, [5] 1 if padded, [6] compiled row width (32,
 * 64 or 128), [7] row blocks per sample, [8] rank columns (8 or 16), [9] LDS bytes per workgroup,
 * [10] 1 if k_mnl_fused fits the shape.  A plan may still fall back (a spilling instantiation, found at plan
 * creation from the code object).  Reads the same environment switches as tr_plan_create.  n_out:
 * entries to write (at most 11).  Returns TR_E_UNSUPPORTED when no factored kernel fits at all.
 */
int tr_mnl_geometry(int64_t I, int64_t J, int R, int C, int32_t* out, int n_out);

/*
 * Device status of the plan's kernels since the last call (synchronises the device).
 * *status = 0: healthy.  Bit 0: a cross-workgroup exchange of the single-pass kernel for wide
 * rows (P beyond one CU's LDS) gave up waiting for a partner workgroup — it happens only when
 * the GPU is shared with another kernel so the cluster was not co-resident (the plan launches at
 * most one workgroup per CU, so an unshared GPU always holds the whole grid); that call's
 * gradient and loss are NaN and the gradient arena's status slot is set.  No reference
 * counterpart (the reference has no device kernels).
 */
int tr_plan_status(tr_plan* plan, int32_t* status);

/*
 * Recover from a device-side failure (status bit set / TR_STOP_DEVICE_ERROR): clears the status
 * and switches the plan to its two-pass path, which has no cross-workgroup dependence.  The fit
 * loop then resumes at the failed iteration from the untouched parameters and Adam state.
 */
int tr_plan_recover(tr_plan* plan);

/*
 * Forward model only (predict path).
 * Replaces lin_model (standard…py:87-130) — out[n] = <X_n, B> + bias — and model
 * (multinomial…py:148-187) — out[n, c] = softmax_c(<X_n, B_c>) — where
 * B = cp_to_tensor((weights, non_neg_fn(Bcp))).
 *   out: n_rows floats (linear) or n_rows x C floats row-major (multinomial).
 */
int tr_forward(tr_plan* plan, const float* X, int64_t n_rows, const float* params,
               const float* weights, float* out, void* stream);

/*
 * Data-term loss and gradient of one sample shard (forward + loss + backward).
 * Replaces the forward, loss_fn and loss.backward() of one fit_Adam iteration
 * (standard…py:460-462; multinomial…py:455-457) — WITHOUT the L2 term, which
 * tr_adam_step / tr_finalize_grad add once after the cross-shard sum.
 *   target      linear: float y[n_rows]; multinomial: int64 labels[n_rows] in [0, C)
 *   class_weight multinomial: float[C] CrossEntropyLoss weights; linear: NULL
 *   norm        linear: global N (MSELoss mean); multinomial: global sum_n cw[y_n]
 *   grad_out    tr_plan_num_grads() floats, overwritten: data gradient of every parameter
 *               (+ bias) and the data loss in the last slot.
 *   yhat_out    optional (may be NULL): linear model output per row (n_rows floats).
 */
int tr_loss_grad(tr_plan* plan, const float* X, int64_t n_rows, const void* target,
                 const float* class_weight, double norm, const float* params,
                 const float* weights, float* grad_out, float* yhat_out,
                 const int32_t* stop_flag, void* stream);

/*
 * L2 term + total loss only (no parameter update) — the closure value/gradient that
 * torch.optim.LBFGS needs in fit() (standard…py:368-373, multinomial…py:357-362).
 *   grad_total_out  num_params floats: data gradient + lambda * d(sum_k ||A_k||_F)/dA
 *   loss_out        1 float: data loss + lambda * sum_k ||A_k||_F (L2_penalty, standard…py:180-196)
 */
int tr_finalize_grad(tr_plan* plan, const float* params, const float* grad,
                     float lambda_l2, float* grad_total_out, float* loss_out, void* stream);

/*
 * One torch.optim.Adam / AMSGrad step on the whole parameter arena, preceded by the L2
 * term and followed by the reference's bookkeeping:
 *   loss_hist[hist_base + iter] = data loss + lambda * L2_penalty   (loss_running.append)
 *   if iter > patience and sum(|diff(loss_hist[iter - patience : hist_base + iter + 1])|) < tol:
 *       *stop_flag = iter + 1                                      (standard…py:467-470)
 * Adam math follows torch/optim/adam.py _single_tensor_adam (torch 2.10):
 *   g += wd * p; m = lerp(m, g, 1 - b1); v = v * b2 + (1 - b2) g^2;
 *   vmax = max(vmax, v) if amsgrad; denom = sqrt(v or vmax) / sqrt(1 - b2^t) + eps;
 *   p -= lr / (1 - b1^t) * m / denom.
 *   step        1-based Adam step t for this iteration
 *   loss_hist   fp64 device array (the reference's loss_running as python floats)
 *   max_exp_avg_sq  may be NULL when amsgrad == 0
 */
int tr_adam_step(tr_plan* plan, float* params, const float* grad, float* exp_avg,
                 float* exp_avg_sq, float* max_exp_avg_sq, float lambda_l2, double lr,
                 double beta1, double beta2, double eps, double weight_decay, int amsgrad,
                 int64_t step, double* loss_hist, int64_t hist_base, int64_t iter,
                 int64_t patience, double tol, int32_t* stop_flag, void* stream);

/*
 * tr_adam_step for torch.optim.Adam with one param group per factor (the hierarchical
 * multinomial module, multinomial_tensor_regression_hierarchical.py:436-440); float32
 * multinomial plans only.  Same arguments and bookkeeping as tr_adam_step, except
 *   lr            n_factors doubles (>= 0), the learning rate of each factor's group; lr 0 keeps
 *                 torch's meaning (the moments advance, the parameters do not move)
 *   n_factors     must equal the plan's number of factors
 *   stepped_mask  bit f set: factor f is in a param group.  A factor outside the mask is a tensor
 *                 the optimizer was never given: its parameters and exp_avg / exp_avg_sq /
 *                 max_exp_avg_sq entries stay bitwise untouched, while its norm still enters the
 *                 recorded loss (and tr_finalize_grad's total gradient is unaffected).
 * All groups share the step count `step`.  With every factor stepped at one lr the result is
 * bitwise tr_adam_step's.  The next-iteration preparation of tr_plan_set_prepare_next is not
 * folded into this step (the following tr_loss_grad prepares its own factors).
 */
int tr_adam_step_groups(tr_plan* plan, float* params, const float* grad, float* exp_avg,
                        float* exp_avg_sq, float* max_exp_avg_sq, float lambda_l2, const double* lr,
                        int n_factors, uint32_t stepped_mask, double beta1, double beta2, double eps,
                        double weight_decay, int amsgrad, int64_t step, double* loss_hist,
                        int64_t hist_base, int64_t iter, int64_t patience, double tol,
                        int32_t* stop_flag, void* stream);

/*
 * Resident fit of the hierarchical multinomial module: ONE workgroup on one CU holds X, the dense
 * coefficient tensor, Z / dZ, the factors and the Adam state in LDS and runs up to 64 complete
 * fit_Adam iterations per launch (forward, double softmax + unweighted CE, X^T dZ, factor gradients,
 * L2 term, the grouped Adam step, loss record, plateau test); parameters and state go back to
 * global memory at the end of the launch.  fp32 fmaf sums in one fixed order, the loss in fp64, no
 * atomics: bitwise reproducible, and independent of how a fit is cut into launches.
 *
 * The envelope: a float32 multinomial plan with exactly two feature modes, n_classes <= 16,
 * rank <= 16, and the LDS image of the plan's max_rows samples within 160 KiB.
 *   tr_mnl_resident_max_rows  the largest n_rows inside the envelope for (I0, I1) features,
 *                             n_classes and rank; 0 when no n_rows fits
 *   tr_plan_set_resident      enable = 1: take the route if the plan is inside the envelope and the
 *                             environment does not say TR_MNL_RESIDENT=0 (a test-facing switch);
 *                             tr_plan_describe then carries "fit=resident".  Outside the envelope
 *                             the call succeeds and the plan stays on the streamed route
 *                             (tr_loss_grad + tr_adam_step_groups).  enable = 0: streamed route.
 *   tr_fit_adam_resident      n_iters (1..64) iterations from loop index `iter`, whose Adam step
 *                             count is `step`, `step + 1`, ...; lr[3] are the learning rates of the
 *                             three factors' param groups, constant over the launch (the caller
 *                             cuts a chunk at a schedule breakpoint).  target: int64 labels.  X is
 *                             read at the plan's row stride.  loss_hist / hist_base / patience / tol /
 *                             stop_flag as tr_adam_step: on a plateau the launch stops after that
 *                             iteration's step and writes *stop_flag = iterations completed.  A
 *                             launch that finds *stop_flag != 0 does nothing.
 */
int64_t tr_mnl_resident_max_rows(int64_t I0, int64_t I1, int n_classes, int rank);
int tr_plan_set_resident(tr_plan* plan, int enable);
int tr_fit_adam_resident(tr_plan* plan, const float* X, int64_t n_rows, const void* target, float* params,
                         const float* weights, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                         float lambda_l2, const double* lr, double beta1, double beta2, double eps,
                         double weight_decay, int amsgrad, int64_t step, int n_iters, double* loss_hist,
                         int64_t hist_base, int64_t iter, int64_t patience, double tol, int32_t* stop_flag,
                         void* stream);

/*
 * Resident sweep: many independent resident fits in one launch, workgroup j fitting member j
 * (a hyperparameter grid: one model per grid point, each with its own data, shape, initial
 * factors and optimizer settings).  No plan is involved.  A member carries the arguments of
 * tr_fit_adam_resident and what that call takes from its plan: the shape (I0, I1, n_classes, rank;
 * inside the envelope above, which is checked per member at its own n_rows), nonneg[3], the
 * softplus beta / threshold and X's row stride in floats (0 = I0 * I1).  Members may differ in
 * every field.  n_iters is 0..64: a member with n_iters = 0 (finished, or shorter than the
 * others) is left untouched, as is one whose *stop_flag is nonzero.  Member j's results are
 * bitwise those of tr_fit_adam_resident on the same inputs.
 *   tr_resident_member_table_bytes  size of the launch's argument table for n_members
 *   tr_fit_adam_resident_many       checks EVERY member before any device call (NULL buffer,
 *                                   n_rows < 1, n_iters outside 0..64, step < 1, iter or
 *                                   hist_base < 0, lr < 0, amsgrad without max_exp_avg_sq:
 *                                   TR_E_ARG; outside the envelope: TR_E_UNSUPPORTED;
 *                                   tr_last_error() names the member's index) and launches
 *                                   nothing if one fails.  table_host (pinned host memory) and
 *                                   table_dev (memory of `device`), each of at least table_bytes >=
 *                                   tr_resident_member_table_bytes(n_members), are the caller's: the
 *                                   table is written to table_host and copied to table_dev on
 *                                   `stream` ahead of the launch, so table_host must not be
 *                                   reused before that copy has completed.
 */
typedef struct tr_resident_member {
  const float* X;        /* (n_rows, I0, I1) at x_row_stride */
  const void* target;    /* int64 labels [n_rows] */
  float* params;         /* (I0 + I1 + n_classes) * rank: the three factors, contiguous */
  const float* weights;  /* [rank] CP component weights */
  float* exp_avg;
  float* exp_avg_sq;
  float* max_exp_avg_sq; /* amsgrad only, else may be NULL */
  double* loss_hist;
  int32_t* stop_flag;
  int64_t n_rows, x_row_stride;
  int64_t I0, I1;
  int32_t n_classes, rank;
  int32_t nonneg[3];
  int32_t amsgrad;
  float softplus_beta, softplus_threshold;
  float lambda_l2;
  int32_t n_iters;
  double lr[3];
  double beta1, beta2, eps, weight_decay;
  int64_t step, hist_base, iter, patience;
  double tol;
} tr_resident_member;

int64_t tr_resident_member_table_bytes(int n_members);
int tr_fit_adam_resident_many(int device, const tr_resident_member* members, int n_members, void* table_host,
                              void* table_dev, int64_t table_bytes, void* stream);

/*
 * Scoring sweep: the forward pass and the metrics of many (model, data set) pairs in one launch
 * (the second half of a hyperparameter grid: every fitted model on its held-out, training and
 * shuffled data).  No plan is involved.  A member is one pair: X (n_rows, I0, I1) float32 at
 * x_row_stride floats (0 = I0 * I1), the three factors contiguous in `params` as in
 * tr_resident_member, the CP component weights, nonneg[3] and the softplus beta / threshold.
 * Outputs, each of which may be NULL:
 *   prob    (n_rows, n_classes) float32: softmax(inner(X, B), dim=1), the module's model() output
 *   pred    int64 [n_rows]: the first index of the row's largest stored prob (numpy's argmax)
 *   counts  int32 [n_classes * n_classes], row-major counts[pred, true]; needs target.  Zeroed by
 *           the call on the stream, then summed with integer atomics (exact in any order)
 *   loss    double [2]: sum_n w[y_n] l_n and sum_n w[y_n], l_n the CrossEntropyLoss of the model()
 *           output (the double softmax the fits record), w = class_weights or 1; needs target and
 *           loss_parts, a scratch of 2 * ceil(n_rows / TR_SCORE_ROW_BLOCK) doubles: one workgroup
 *           scores TR_SCORE_ROW_BLOCK rows, and the workgroups' fp64 partial sums are added in
 *           block order by a second small kernel
 * Labels outside [0, n_classes) are the caller's to refuse; such a row is left out of counts and loss.
 * The envelope: n_classes <= 16, rank <= 16 and the LDS image (the dense P x C coefficient tensor
 * and the factors) within 160 KiB; it contains every shape for which tr_mnl_resident_max_rows >= 1,
 * and n_rows is any value >= 1 (X streams from global memory; one call takes at most 4194303 row
 * blocks over all members, the grid HIP accepts, else TR_E_UNSUPPORTED).  fp32 fmaf sums in one fixed order,
 * no floating-point atomics: a member's results are bitwise reproducible and independent of the
 * other members of the table.
 *   tr_mnl_score_envelope        1 inside the envelope, 0 outside
 *   tr_score_member_table_bytes  size of the launch's argument table for n_members
 *   tr_mnl_score_many            checks EVERY member before any device call (NULL X, params or
 *                                weights, n_rows < 1, a negative stride, counts or loss without
 *                                target, loss without loss_parts: TR_E_ARG; outside the envelope:
 *                                TR_E_UNSUPPORTED; tr_last_error() names the member's index) and
 *                                launches nothing if one fails.  table_host (pinned) and table_dev as
 *                                in tr_fit_adam_resident_many.  n_members == 0 succeeds.
 */
#define TR_SCORE_ROW_BLOCK 256

typedef struct tr_score_member {
  const float* X;             /* (n_rows, I0, I1) at x_row_stride */
  const void* target;         /* int64 labels [n_rows], or NULL */
  const float* params;        /* (I0 + I1 + n_classes) * rank: the three factors, contiguous */
  const float* weights;       /* [rank] CP component weights */
  const float* class_weights; /* [n_classes], or NULL (every class at 1) */
  float* prob;
  int64_t* pred;
  int32_t* counts;
  double* loss;
  double* loss_parts;         /* scratch, needed with loss */
  int64_t n_rows, x_row_stride;
  int64_t I0, I1;
  int32_t n_classes, rank;
  int32_t nonneg[3];
  float softplus_beta, softplus_threshold;
} tr_score_member;

int tr_mnl_score_envelope(int64_t I0, int64_t I1, int n_classes, int rank);
int64_t tr_score_member_table_bytes(int n_members);
int tr_mnl_score_many(int device, const tr_score_member* members, int n_members, void* table_host,
                      void* table_dev, int64_t table_bytes, void* stream);

/*
 * Shared-X linear sweep: up to 16 CP linear models with two feature modes (a hyperparameter grid:
 * one model per grid point) fitted over ONE X (n_rows, I0, I1) float32 at x_row_stride floats
 * (0 = I0 * I1; a stride below I0 * I1 is a windowed view).  No plan is involved.  With dense
 * coefficient tensors the members' forward passes are one skinny GEMM over X and their gradient
 * passes another, so an iteration reads X twice whatever the number of members, and the number of
 * kernel launches per iteration (8) does not depend on it either.  Members differ in rank,
 * nonneg[2], softplus settings, weights, target, lambda and every optimizer setting.
 * The envelope: P = I0 * I1 and the row stride multiples of 4 floats, X 16-byte aligned, rank 1..32,
 * I0, I1 <= 2^20, P <= 2^30; any n_rows >= 1.
 * A member's `params` is its plan arena (factor 0, factor 1, bias), `grad` its gradient arena of
 * (I0 + I1) * rank + 3 floats, laid out as tr_loss_grad leaves it (factor gradients, bias gradient,
 * data loss, status).  exp_avg / exp_avg_sq / max_exp_avg_sq / loss_hist / stop_flag / step /
 * hist_base / iter / patience / tol are those of tr_adam_step; n_iters is how many iterations the
 * call runs for this member (tr_linear_many_step: 0 or 1; tr_linear_many_fit: 0..64).  A member
 * whose *stop_flag is nonzero or whose n_iters is used up is left untouched: parameters, Adam
 * state and loss history (its grad arena is scratch).
 * No floating-point atomics and fixed summation orders that depend on (n_rows, I0, I1) alone: a
 * member's results are bitwise reproducible and depend neither on the other members nor on its
 * position in the table.  Given the same gradient bits the update is tr_adam_step's, bit for bit.
 *   tr_linear_many_envelope        1 inside the envelope, 0 outside; needs no device
 *   tr_linear_many_workspace_bytes size of the caller's device workspace (<= 0: outside the envelope)
 *   tr_linear_member_table_bytes   size of the argument table for n_members
 *   tr_linear_many_loss_grad       one evaluation: fills every member's grad arena
 *   tr_linear_many_step            the update of every member with n_iters = 1 from its grad arena
 *   tr_linear_many_fit             max(n_iters) iterations of both
 * Every entry checks the shape and EVERY member before any device call (NULL buffer, n_iters out of
 * range, step < 1, iter or hist_base < 0, lr < 0, amsgrad without max_exp_avg_sq, more than 16
 * members: TR_E_ARG; outside the envelope: TR_E_UNSUPPORTED; tr_last_error() names the member's
 * index) and launches nothing if one fails.  n_members == 0 succeeds.  table_host (pinned) and
 * table_dev as in tr_fit_adam_resident_many.
 */
typedef struct tr_linear_member {
  float* params;         /* (I0 + I1) * rank + 1: factor 0, factor 1, bias */
  const float* weights;  /* [rank] CP component weights */
  const float* y;        /* [n_rows] targets */
  float* exp_avg;
  float* exp_avg_sq;
  float* max_exp_avg_sq; /* amsgrad only, else may be NULL */
  float* grad;           /* (I0 + I1) * rank + 3 */
  double* loss_hist;
  int32_t* stop_flag;
  int32_t rank;
  int32_t nonneg[2];
  int32_t amsgrad;
  float softplus_beta, softplus_threshold;
  float lambda_l2;
  int32_t n_iters;
  double lr, beta1, beta2, eps, weight_decay;
  int64_t step, hist_base, iter, patience;
  double tol;
} tr_linear_member;

int tr_linear_many_envelope(int64_t I0, int64_t I1, int64_t x_row_stride, int rank);
int64_t tr_linear_many_workspace_bytes(int64_t n_rows, int64_t I0, int64_t I1, int n_members);
int64_t tr_linear_member_table_bytes(int n_members);
int tr_linear_many_loss_grad(int device, const float* X, int64_t n_rows, int64_t x_row_stride, int64_t I0, int64_t I1,
                             const tr_linear_member* members, int n_members, void* workspace,
                             int64_t workspace_bytes, void* table_host, void* table_dev, int64_t table_bytes,
                             void* stream);
int tr_linear_many_step(int device, int64_t I0, int64_t I1, const tr_linear_member* members, int n_members,
                        void* table_host, void* table_dev, int64_t table_bytes, void* stream);
int tr_linear_many_fit(int device, const float* X, int64_t n_rows, int64_t x_row_stride, int64_t I0, int64_t I1,
                       const tr_linear_member* members, int n_members, void* workspace, int64_t workspace_bytes,
                       void* table_host, void* table_dev, int64_t table_bytes, void* stream);

/*
 * Scoring the shared-X linear sweep: up to 16 CP linear models with two or three feature modes scored
 * over ONE X (n_rows, dims[0], .., dims[n_modes - 1]) float32 at x_row_stride floats (0 = P, the
 * product of the dims).  Only the forward half of the sweep runs: X is read once and the call makes
 * five kernel launches whatever the number of members.  Per member, yhat = <X, B> + bias goes to
 * `yhat` when that is not NULL, and with a target `y` five fp64 sums go to `sums`:
 *   sums[0] = sum e^2 (e = yhat - y), sums[1] = sum (yhat - k), sums[2] = sum (yhat - k)^2,
 *   sums[3] = sum (y - k), sums[4] = sum (y - k)^2, with the shift k = y[0]
 * from which the MSE, the variances and R^2 follow without cancellation.  `params` holds the factors
 * in mode order, then the bias (tr_linear_member's arena order).
 * The envelope: 2 or 3 modes, P and the row stride multiples of 4 floats, X 16-byte aligned, rank
 * 1..32, every dim <= 2^20, P <= 2^30; any n_rows >= 1.  For two modes the forward's split of
 * (n_rows, P) is the fit's, so yhat and sums[0] carry the bits tr_linear_many_loss_grad works with.
 * No floating-point atomics; every order depends on the shape alone and a member's bits depend
 * neither on the other members nor on its position.
 * The shape and EVERY member are checked before any device call (NULL params or weights, y without
 * sums, neither yhat nor y, more than 16 members: TR_E_ARG; rank or shape outside the envelope:
 * TR_E_UNSUPPORTED; tr_last_error() names the member).  n_members == 0 succeeds.
 */
typedef struct tr_linear_score_member {
  const float* params;   /* sum(dims) * rank + 1: the factors in mode order, then the bias */
  const float* weights;  /* [rank] CP component weights */
  const float* y;        /* [n_rows] targets; NULL: predict only */
  float* yhat;           /* [n_rows]; NULL: not wanted */
  double* sums;          /* [5], required with y */
  int32_t rank;
  int32_t nonneg[3];
  float softplus_beta, softplus_threshold;
} tr_linear_score_member;

int tr_linear_score_envelope(int n_modes, const int64_t* dims, int64_t x_row_stride, int rank);
int64_t tr_linear_score_workspace_bytes(int64_t n_rows, int n_modes, const int64_t* dims, int n_members);
int64_t tr_linear_score_table_bytes(int n_members);
int tr_linear_many_score(int device, const float* X, int64_t n_rows, int64_t x_row_stride, int n_modes,
                         const int64_t* dims, const tr_linear_score_member* members, int n_members, void* workspace,
                         int64_t workspace_bytes, void* table_host, void* table_dev, int64_t table_bytes,
                         void* stream);

/*
 * Shared-X multinomial sweep: CP multinomial models with two feature modes and a class factor (a
 * hyperparameter grid: one model per grid point) fitted over ONE X (n_rows, I0, I1) float32 at
 * x_row_stride floats (0 = I0 * I1; a stride below I0 * I1 is a windowed view).  No plan is involved.
 * A member with C classes is C columns of a dense coefficient matrix; the members of a call hold at
 * most 64 columns in total (four 16-column MFMA tiles: 12 members at C = 5, 4 at C = 16).  Member j
 * owns the columns col0_j .. col0_j + C_j - 1, col0 the running sum of the class counts.  The forward
 * passes are one skinny GEMM over X and the gradient passes another, so an iteration reads X twice
 * whatever the number of members, and the number of kernel launches per iteration (9) does not depend
 * on it either.  Members differ in labels, class count, rank, nonneg[3], softplus settings, CP
 * weights, class weights, lambda and every optimizer setting.
 * The loss is the module's: CrossEntropyLoss(weight) on the softmax output (the double softmax),
 * sum_n cw[y_n] l_n / cw_norm with cw_norm = sum_n cw[y_n].
 * The envelope: P = I0 * I1 and the row stride multiples of 4 floats, X 16-byte aligned, n_classes
 * 2..16, rank 1..32, I0, I1 <= 2^20, P <= 2^28; any n_rows >= 1.
 * A member's `params` is its plan arena (factor 0, factor 1, class factor), `grad` its gradient arena
 * of (I0 + I1 + n_classes) * rank + 2 floats, laid out as tr_loss_grad leaves it (factor gradients,
 * data loss, status).  The Adam, history and stop fields are those of tr_linear_member.  A member
 * whose *stop_flag is nonzero or whose n_iters is used up is left untouched: parameters, Adam state
 * and loss history (its grad arena is scratch).
 * No floating-point atomics and fixed summation orders that depend on (n_rows, I0, I1) alone: a
 * member's results are bitwise reproducible and depend neither on the other members, nor on its
 * columns' position, nor on the number of tiles in use.  Given the same gradient bits the update is
 * tr_adam_step's, bit for bit.
 *   tr_mnl_many_envelope           1 inside the envelope, 0 outside; needs no device
 *   tr_mnl_many_workspace_bytes    size of the caller's device workspace (<= 0: outside the envelope)
 *   tr_mnl_many_member_table_bytes size of the argument table for n_members
 *   tr_mnl_many_loss_grad          one evaluation: fills every member's grad arena
 *   tr_mnl_many_step               the update of every member with n_iters = 1 from its grad arena
 *   tr_mnl_many_fit                max(n_iters) iterations of both
 * Every entry checks the shape and EVERY member before any device call (NULL buffer, n_iters out of
 * range, step < 1, iter or hist_base < 0, lr < 0, cw_norm <= 0, amsgrad without max_exp_avg_sq, more
 * than 64 columns in total: TR_E_ARG; outside the envelope: TR_E_UNSUPPORTED; tr_last_error() names
 * the member's index) and launches nothing if one fails.  n_members == 0 succeeds.  table_host
 * (pinned) and table_dev as in tr_fit_adam_resident_many.
 */
typedef struct tr_mnl_many_member {
  float* params;              /* (I0 + I1 + n_classes) * rank: factor 0, factor 1, class factor */
  const float* weights;       /* [rank] CP component weights */
  const int64_t* y;           /* [n_rows] labels in 0..n_classes-1 */
  const float* class_weights; /* [n_classes] */
  float* exp_avg;
  float* exp_avg_sq;
  float* max_exp_avg_sq;      /* amsgrad only, else may be NULL */
  float* grad;                /* (I0 + I1 + n_classes) * rank + 2 */
  double* loss_hist;
  int32_t* stop_flag;
  double cw_norm;             /* sum_n class_weights[y_n] */
  int32_t n_classes, rank;
  int32_t nonneg[3];
  int32_t amsgrad;
  float softplus_beta, softplus_threshold;
  float lambda_l2;
  int32_t n_iters;
  double lr, beta1, beta2, eps, weight_decay;
  int64_t step, hist_base, iter, patience;
  double tol;
} tr_mnl_many_member;

int tr_mnl_many_envelope(int64_t I0, int64_t I1, int64_t x_row_stride, int n_classes, int rank);
int64_t tr_mnl_many_workspace_bytes(int64_t n_rows, int64_t I0, int64_t I1);
int64_t tr_mnl_many_member_table_bytes(int n_members);
int tr_mnl_many_loss_grad(int device, const float* X, int64_t n_rows, int64_t x_row_stride, int64_t I0, int64_t I1,
                          const tr_mnl_many_member* members, int n_members, void* workspace,
                          int64_t workspace_bytes, void* table_host, void* table_dev, int64_t table_bytes,
                          void* stream);
int tr_mnl_many_step(int device, int64_t I0, int64_t I1, const tr_mnl_many_member* members, int n_members,
                     void* table_host, void* table_dev, int64_t table_bytes, void* stream);
int tr_mnl_many_fit(int device, const float* X, int64_t n_rows, int64_t x_row_stride, int64_t I0, int64_t I1,
                    const tr_mnl_many_member* members, int n_members, void* workspace, int64_t workspace_bytes,
                    void* table_host, void* table_dev, int64_t table_bytes, void* stream);

/*
 * Fold the NEXT iteration's factor preparation into tr_adam_step: with enable = 1, on a plan
 * that takes the factored multinomial single pass, every tr_adam_step also computes
 * softplus(A_k) and its derivative from the parameters it has just written, and the following
 * tr_loss_grad on the SAME params pointer skips its own preparation launch.  Valid as long as
 * the parameters change only through tr_adam_step between those calls (the fit_Adam loop);
 * results are bitwise identical to enable = 0.  Other plans ignore the setting.
 */
int tr_plan_set_prepare_next(tr_plan* plan, int enable);

/*
 * float64 linear model: CP_linear_regression(..., dtype=torch.float64) (standard…py:206; the
 * reference's KAT-1, demo_TensorRegression.ipynb, is an fp64 LBFGS fit).  Same arenas and
 * semantics as the fp32 entry points above with double buffers (X, y, params, weights, grad,
 * Adam state, outputs); the plan computes in double (two passes over X on the VALU).  A float64
 * plan accepts only the _f64 entry points, a float32 plan only the float ones (TR_E_ARG).
 */
int tr_plan_create_f64(tr_plan** out, int device, int n_feature_modes, const int64_t* feature_dims, int rank,
                       int64_t max_rows, const int32_t* non_negative, double softplus_beta,
                       double softplus_threshold);
int tr_forward_f64(tr_plan* plan, const double* X, int64_t n_rows, const double* params, const double* weights,
                   double* out, void* stream);
int tr_loss_grad_f64(tr_plan* plan, const double* X, int64_t n_rows, const double* y, double norm,
                     const double* params, const double* weights, double* grad_out, double* yhat_out,
                     const int32_t* stop_flag, void* stream);
int tr_finalize_grad_f64(tr_plan* plan, const double* params, const double* grad, double lambda_l2,
                         double* grad_total_out, double* loss_out, void* stream);
int tr_adam_step_f64(tr_plan* plan, double* params, const double* grad, double* exp_avg, double* exp_avg_sq,
                     double* max_exp_avg_sq, double lambda_l2, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int amsgrad, int64_t step, double* loss_hist, int64_t hist_base,
                     int64_t iter, int64_t patience, double tol, int32_t* stop_flag, void* stream);

/*
 * Spectral model plan (spectral_tensor_regression.CP_linear_regression, spectral…py:424-539;
 * fit model lin_model :118-165 + stepwise_spectral_model :339-390; predict model
 * lin_model + spectral_model :168-220).  X is (N, n_w, n_d) fp32, y is (N, n_out) fp32.
 *   n_complex      = n_complex_dim + 1 (third dim of Bcp_c[0])
 *   non_negative   host int32[3]: flags of the (w, d, out) factors, shared by Bcp_n and Bcp_c
 * Parameter arena (reference order Bcp_n + Bcp_c + [bias], each row-major):
 *   A0 (n_w, Rn) | A1 (n_d, Rn) | A2 (n_out, Rn) | C0 (n_w, Rs, n_complex) | C1 (n_d, Rs) |
 *   C2 (n_out, Rs) | bias (n_out)
 * tr_plan_factor_offset(plan, f) gives f = 0..5 and the bias offset for f = 6.
 * With such a plan:
 *   tr_loss_grad   target = y (N x n_out floats), norm = global N * n_out (MSELoss mean),
 *                  class_weight = NULL, yhat_out (optional) = fit-model y_hat (N x n_out)
 *   tr_forward     out (N x n_out) = the reference's predict() model (spectral…py:959-960);
 *                  weights = all rank_normal + rank_spectral weights
 *   tr_adam_step   also applies the spectral NaN stop (spectral…py:738-741): when the loss
 *                  is NaN and iter <= patience, *stop_flag = -(iter + 1) (stopped, not converged)
 * Envelope (tr_plan_create_spectral returns TR_E_UNSUPPORTED outside it, with the reason in
 * tr_last_error()):  K = rank_normal + rank_spectral * n_complex <= 256, n_w <= 2^24,
 * n_d, n_out <= 2^16, and one sample's epilogue — n_d * (K + 1) + (n_d + n_out) *
 * (rank_normal + rank_spectral) floats (+ scratch) — within the 160 KiB LDS of a CU.  Inside it
 * the plan picks (tr_plan_describe):
 *   slice-1pass-mfma   training at n_w = 256, 97 <= n_d <= 130 (n_d >= 128 or n_d % 4 == 0),
 *                      1 <= Rn <= 16, Rs * n_complex <= 16 with n_complex in {1, 2, 4},
 *                      n_out <= 64 (and its LDS fits): column-slice single pass (config 5);
 *                      described as slice-1pass-mfma-bf16split when its GEMMs run on the bf16
 *                      matrix cores through split operands (the default): factor-side operands in
 *                      three round-to-nearest bf16 pieces (exact), the sample data in two
 *                      (|x - x1 - x2| < 2^-16 |x|, measured 2^-17, unbiased), fp32 accumulation.  At full config-5
 *                      size its gradients lie within 3.5e-7 normwise of an fp64 closed form (the
 *                      f32 MFMA form 1.1e-7, the reference's own fp32 op sequence 0.6-4.2e-6);
 *                      results are not bitwise those of the f32 MFMA form.  Environment, read at
 *                      plan creation: TR_SLICE_XPIECES=3 takes the sample data in three pieces too
 *                      (exact; slower), TR_SLICE_SPLIT=0 the f32 MFMA form
 *   fused-1pass-mfma   K <= 32, n_w, n_d, n_out <= 256 and the whole sample + scratch in LDS:
 *                      single pass; also every tr_forward / tr_spectral_latents of such a plan
 *   generic-3kernel-mfma  any other shape in the envelope: T_n staged through HBM (three kernels)
 */
int tr_plan_create_spectral(tr_plan** out, int device, int64_t n_w, int64_t n_d, int64_t n_out,
                            int rank_normal, int rank_spectral, int n_complex, int64_t max_rows,
                            const int32_t* non_negative, float softplus_beta, float softplus_threshold);

/*
 * stepwise_latents_model (spectral…py:284-336) — out (N x rank_normal) =
 * einsum('tdr,drs->tr', einsum('twd,wrs->tdr', X, phi(A0)), phi(A1)); used by predict_latents.
 */
int tr_spectral_latents(tr_plan* plan, const float* X, int64_t n_rows, const float* params, float* out,
                        void* stream);

/*
 * Convolutional spectral model plan (ABI 9; convolutional_spectral_tensor_regression.
 * CP_linear_regression, …py:750-877; model conv_linear :650-678 = conv :259-290 + complex_magnitude
 * :292-303 + slmm_helper :426-430).  X is the untiled (T, n_d) fp32 series, y is (T, n_out); with
 * T' = T - n_w + 1 and phi = softplus on flagged factors:
 *   z[t,d,k] = sum_w X[t+w,d] phi(K)[w,k],  u = z (one component, signed) or ||z[t,d,s,:]||_2,
 *   y_hat[t,n] = sum_r (sum_d u[t,d,r] phi(Bd)[d,r]) phi(Bo)[n,r] + bias[n],   t in [0, T')
 *   n_w            temporal_window (odd);  n_complex = n_complex_dim + 1
 *   max_series_rows  largest T later passed as n_rows
 *   non_negative   host int32[3]: flags of (w, d, out); the w flag covers Kn and Ks
 * Parameter arena (the reference's optimizer order Bcp_n + Bcp_w + [bias], each row-major):
 *   Bd (n_d, R) | Bo (n_out, R) | Kn (n_w, Rn) | Ks (n_w, Rs, n_complex) | bias (n_out),  R = Rn + Rs
 * tr_plan_factor_offset(plan, f) gives f = 0..3 and the bias offset for f = 4.
 * With such a plan:
 *   tr_forward     n_rows = T; out is (T' x n_out); weights is ignored (the reference's model never
 *                  uses them) but must not be NULL
 *   tr_loss_grad   n_rows = T; target = the T' x n_out block of y that starts at row n_w / 2
 *                  (y[idx_conv]); norm = global T' * n_out; yhat_out (optional) is T' x n_out
 *   tr_finalize_grad / tr_adam_step   ignore their lambda_l2 argument and take one lambda per
 *                  factor group from tr_plan_set_l2_weights (required first): the total is
 *                  loss + l[0] (||Kn|| + ||Ks||) + l[1] ||Bd|| + l[2] ||Bo|| (…py:1046); tr_adam_step
 *                  also applies the NaN stop (…py:1059-1062) like a spectral plan
 * Bad arguments (even or non-positive n_w, R outside 1..32, n_complex outside 1..4, n_out > 64,
 * NULL pointers) return TR_E_ARG before any device call; shapes beyond the kernel's envelope
 * (n_w > 257, n_d > 2^16, Rn + Rs * n_complex > 64) return TR_E_UNSUPPORTED with the reason in
 * tr_last_error().  tr_plan_describe names the kernel form (path=conv-1pass-fmaf: one pass, fp32
 * fmaf; X rows may start at any float offset and use any row stride >= n_d).
 */
int tr_plan_create_conv(tr_plan** out, int device, int64_t n_w, int64_t n_d, int64_t n_out, int rank_normal,
                        int rank_spectral, int n_complex, int64_t max_series_rows, const int32_t* non_negative,
                        float softplus_beta, float softplus_threshold);

/* The conv plan's L2 weights: lambdas[3] = (w, d, out) as fit_Adam's lambda_L2 (host array, n = 3).
 * Also taken by a conv phase plan and a conv Fourier plan (below).  TR_E_ARG on a NULL plan or a plan
 * of another model. */
int tr_plan_set_l2_weights(tr_plan* plan, const float* lambdas, int n);

/*
 * Phase-constrained spectral convolutional model plan (an addition within ABI 9: no existing
 * prototype or struct changes; phase_constrained_spectral_convolutional_tensor_regression.
 * CP_linear_regression, …py:1034-1181; model forward_model :696-744 with phase_shifter :959-1027).
 * The conv plan above with two spectral components of which the second is derived: a spectral rank
 * carries one kernel and its pair is that kernel with every frequency shifted by 90 degrees,
 *   z0 = X * phi(Ks),  z1 = X * H phi(Ks),  u_s = sqrt(z0^2 + z1^2),
 *   (H k)[n] = sum_m h[(n - m) mod W] k[m],  h[d] = (2 / W) sum_{j=1..(W-1)/2} sin(2 pi j d / W)
 * (H acts after the softplus; h is computed in fp64 with the exact pi/2 and rounded once).
 * Arguments as tr_plan_create_conv without n_complex.  Parameter arena:
 *   Bd (n_d, R) | Bo (n_out, R) | Kn (n_w, Rn) | Ks (n_w, Rs) | bias (n_out),  R = Rn + Rs
 * tr_plan_factor_offset(plan, f) gives f = 0..3 and the bias offset for f = 4.
 * With such a plan tr_forward, tr_loss_grad, tr_plan_num_params and tr_plan_num_grads carry the conv
 * plan's meaning; tr_finalize_grad / tr_adam_step (with the NaN stop) need tr_plan_set_l2_weights
 * and tr_plan_set_smoothness first and record the reference's total (…py:1412)
 *   loss + l[0] (||Kn|| + ||Ks||) + l[1] ||Bd|| + l[2] ||Bo|| + sum_{F in (Kn, Ks), F non-empty}
 *   lambda_smooth * mean((Delta^q F)^2),
 * Delta^q = q rounds of a first difference with one zero row before and after (W + q rows).
 * Same TR_E_ARG / TR_E_UNSUPPORTED split as tr_plan_create_conv (with R <= 32 the pair columns
 * Rn + 2 Rs never exceed 64).  tr_plan_describe reports path=conv-1pass-fmaf+phase.
 */
#define TR_MODEL_CONV_PHASE 4
int tr_plan_create_conv_phase(tr_plan** out, int device, int64_t n_w, int64_t n_d, int64_t n_out, int rank_normal,
                              int rank_spectral, int64_t max_series_rows, const int32_t* non_negative,
                              float softplus_beta, float softplus_threshold);

/* The conv phase plan's smoothness term: lambda_smooth and smooth_diff_order (0..8) of fit / fit_Adam.
 * Also taken by a conv Fourier plan (below).  TR_E_ARG on a NULL plan, a plan of another model or a
 * diff_order outside 0..8. */
int tr_plan_set_smoothness(tr_plan* plan, float lambda_smooth, int diff_order);

/*
 * Convolutional Fourier model plan (an addition within ABI 9: no existing prototype or struct
 * changes; convolutional_fourier_tensor_regression.CP_linear_regression, …py:909-1050; model
 * forward_model :694-725).  The conv plan's model (unconstrained Ks (n_w, Rs, n_complex), magnitude
 * over the components) with the phase plan's smoothness term and the output-spectrum penalty.
 * Arguments, parameter arena, TR_E_ARG / TR_E_UNSUPPORTED split and envelope are those of
 * tr_plan_create_conv.  tr_plan_set_l2_weights and tr_plan_set_smoothness accept the plan and are
 * both required before tr_finalize_grad / tr_adam_step, which record the reference's total (:1281)
 *   ((((loss_rec + L2_w) + L2_n) + loss_spectral) + loss_smoothness),
 * the smoothness term over Kn and Ks with Ks seen as (n_w, Rs * n_complex); stops as a phase plan.
 * tr_plan_describe reports path=conv-1pass-fmaf+fourier, and +spectrum-dft while the penalty is on.
 */
#define TR_MODEL_CONV_FOURIER 5
int tr_plan_create_conv_fourier(tr_plan** out, int device, int64_t n_w, int64_t n_d, int64_t n_out, int rank_normal,
                                int rank_spectral, int n_complex, int64_t max_series_rows,
                                const int32_t* non_negative, float softplus_beta, float softplus_threshold);

/*
 * The output-spectrum penalty of a conv Fourier plan (spectral_penalty, …py:727-812):
 *   Y = rfft(y_hat, n_fft) (y_hat zero-padded from T' rows), A = |Y| (F = n_fft / 2 + 1 bins),
 *   M[j] = sum_{s < n_kernel} A[j + s] g[s] (Fs = F - n_kernel + 1 rows), M_y the same of the target,
 *   pen = lambda * mean(((M - M_y) / (M_y + 1e-8))^2).
 * The transform is a direct real DFT of any length with exact integer angle indices (twiddles from an
 * n_fft-entry table computed in fp64); every sum has one fixed order.
 *   kernel_host   host float[n_kernel]: g; n_kernel = 0 turns the penalty off (the other arguments
 *                 are then ignored); n_kernel <= 4097
 *   n_fft         transform length, 1 <= n_fft <= 2^22
 *   target_dev    device (n_rows x n_out) series whose smoothed spectrum M_y is computed here (on
 *                 `stream`) and kept
 * Sizes the spectrum workspace (counted by tr_plan_workspace_bytes).  While the penalty is on,
 * tr_loss_grad runs k_conv forward -> DFT -> spectrum terms -> adjoint DFT -> k_conv with the
 * penalty's gradient added to the residual; its loss slot keeps loss_rec alone, the penalty value
 * stays in a plan-owned device scalar that the update step adds, and n_rows - n_w + 1 <= n_fft is
 * required.  TR_E_ARG on a NULL plan, a plan of another model, n_rows > n_fft, n_rows < 1,
 * n_fft / 2 + 1 < n_kernel, or NULL pointers with n_kernel > 0.
 */
int tr_plan_set_spectrum_penalty(tr_plan* plan, float lambda, const float* kernel_host, int n_kernel, int64_t n_fft,
                                 const float* target_dev, int64_t n_rows, void* stream);

/* The smoothed magnitude spectrum M (Fs x n_out) of a device series (n_rows x n_out, n_rows <= n_fft)
 * with the plan's g and n_fft.  TR_E_ARG without tr_plan_set_spectrum_penalty (n_kernel > 0) first. */
int tr_conv_spectrum(tr_plan* plan, const float* series_dev, int64_t n_rows, float* out_dev, void* stream);

/* The penalty value (one float) and d pen / d series (n_rows x n_out) of a device series: the stages
 * tr_loss_grad runs between its two X passes. */
int tr_conv_spectrum_penalty(tr_plan* plan, const float* series_dev, int64_t n_rows, float* value_out_dev,
                             float* grad_out_dev, void* stream);

/*
 * Per-kernel device timing (measurement support; no reference counterpart).
 * `enable` is a bit mask over TR_KERNEL_* kinds (1 << kind; -1 = all): every launch of a
 * selected kind is bracketed by hipEvents on the caller's stream (no host synchronisation).  tr_plan_read_timing synchronises the recorded events and returns,
 * per kernel kind (TR_KERNEL_*), the summed elapsed milliseconds and the number of launches,
 * then clears the record.  tr_plan_set_timing_every(plan, n) brackets only the n-th, 2n-th, ...
 * launch of each selected kind (n >= 1, default 1; tr_plan_set_timing restarts the count), for
 * runs that must disturb the stream even less.  The events are timing-only (no system-scope
 * fence when recorded).
 */
#define TR_KERNEL_STREAM_FUSED 0 /* single-pass X stream (linear) */
#define TR_KERNEL_STREAM_ROWS 1  /* two-pass forward X stream */
#define TR_KERNEL_STREAM_COLS 2  /* two-pass backward X stream */
#define TR_KERNEL_REDUCE 3       /* slab reduction */
#define TR_KERNEL_MTTKRP 4       /* factor gradients */
#define TR_KERNEL_PREP 5         /* softplus + dense B */
#define TR_KERNEL_UPDATE 6       /* L2 + Adam + plateau test */
#define TR_KERNEL_NKINDS 7
int tr_plan_set_timing(tr_plan* plan, int enable);
int tr_plan_set_timing_every(tr_plan* plan, int every);
int tr_plan_read_timing(tr_plan* plan, double* total_ms /* [TR_KERNEL_NKINDS] */,
                        int64_t* launches /* [TR_KERNEL_NKINDS] */);

#ifdef __cplusplus
}
#endif

#endif /* TENSOR_REGRESSION_HIP_H */
