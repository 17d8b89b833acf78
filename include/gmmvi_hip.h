/*
 * gmmvi_hip.h -- C ABI of libgmmvi_hip.so: the MI355X (gfx950) implementation of the per-iteration hot path
 * of OlegArenz/gmmvi (GMMVI.train_iter(): sample selection + background density -> model log-density/gradient
 * -> Stein/MORE natural-gradient estimate -> per-component KL-constrained update -> weight update).
 *
 * The reference has no FFI: its boundary for this path is the Python plug-in surface of
 * src/gmmvi/optimization/gmmvi.py:163-174 and the modules it calls.  Each entry point below names the
 * reference call site (path:line relative to /root/reference/src/gmmvi) whose arithmetic it replaces; the
 * Python classes in gmmvi_amd/ keep the reference's names and argument order and bind these symbols through
 * ctypes (INTEGRATION.md shows the binding a maintainer of the reference would add).
 *
 * Conventions
 *   - plain C: pointers and sizes only, no C++/torch types, no exceptions across the boundary;
 *   - every function returns 0 on success, a negative gmmvi_status otherwise; gmmvi_last_error() gives text;
 *   - numerical rejection (non-positive Cholesky pivot, NaN) is reported through success[] outputs, never as
 *     an error code (reference: NaN-Cholesky -> rejected update, ng_based_component_updater.py:320-324,:493);
 *   - all array arguments are DEVICE pointers obtained from gmmvi_malloc (names end in _dev) unless the
 *     parameter is documented as host; arrays are dense row-major fp32 (int32 for indices/flags);
 *   - calls are asynchronous on the context's HIP stream; gmmvi_download / gmmvi_sync synchronise;
 *   - one context per device per process; a context is not thread-safe (the reference caller is single
 *     threaded).
 */
#ifndef GMMVI_HIP_H
#define GMMVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gmmvi_ctx gmmvi_ctx;

enum gmmvi_status {
    GMMVI_OK = 0,
    GMMVI_ERR_HIP = -1,        /* a HIP runtime call failed */
    GMMVI_ERR_ARG = -2,        /* invalid argument / unsupported shape */
    GMMVI_ERR_RCCL = -3,       /* an RCCL call failed */
    GMMVI_ERR_STATE = -4       /* call not valid in the context's current state */
};

enum gmmvi_family {
    GMMVI_GAUSS = 0,           /* log N(x; m, L L^T)                           models/full_cov_gmm.py:56-62 */
    GMMVI_STUDENT_T = 1        /* multivariate Student-t, scale operator L     target_distributions/student_t_mixture.py:40-44 */
};

enum gmmvi_stein_flags {
    GMMVI_SELF_NORMALIZED = 1, /* ng_estimator.py:171-188 (else :154-169, not symmetrised) */
    GMMVI_OWN_SAMPLES_ONLY = 2, /* ng_estimator.py:110-118 */
    /* gmmvi_train_iter_samtron only: finish the estimate as gmmvi_stein does (H, g materialised) instead of forming the
     * whitened matrix of the component update directly from the moment sums (same mathematics, different rounding) */
    GMMVI_EXPLICIT_ESTIMATE = 4
};

#define GMMVI_MORE_REGISTER_MAX_DIM 21  /* gmmvi_more: up to here the F x F ridge system (F = D(D+1)/2 + D + 1) is factorised in
                                         * one workgroup's registers; above (D <= 63; components of a blocked-path dimension are re-packed for the call) a tiled Gram launch and a blocked fp64
                                         * Cholesky in global memory take over */
#define GMMVI_MORE_BLOCKED_MAX_DIM 128 /* gmmvi_more_blocked: 64 <= D <= 128 from the blocked component layout */
#define GMMVI_MORE_DIAG_MAX_DIM 1024   /* gmmvi_more_diag: diagonal-covariance mixtures, 1 <= D <= 1024 (F = 2 D + 1 features) */
#define GMMVI_MAX_DIM 64       /* register-resident kernels exist for D <= 64; they are used for D <= 50 (environment
                                * GMMVI_BLOCKED_ABOVE, 16..64, moves that threshold) */
#define GMMVI_MAX_DIM_BLOCKED 512   /* above the threshold, D <= 512: blocked kernels (dense L^-1 blocks, fp32 MFMA contractions)
                                     * behind gmmvi_packed_stride / pack_components / cholesky / mixture_eval(_dual) /
                                     * sample_components / stein / update_components_kl / _direct / _iblr */
#define GMMVI_MAX_DIM_DIAG 131072   /* diagonal-covariance mixtures, 1 <= D <= 131072: the O(D) kernels of csrc/diag_sweep.hip and the
                                     * component updates of csrc/diag.hip (one wavefront per component up to GMMVI_MAX_DIM_BLOCKED, one
                                     * workgroup per component above).  gmmvi_diag_embed / _extract build [K,D,D] and stay at
                                     * GMMVI_MAX_DIM_BLOCKED */

/* ---- context, errors, memory ------------------------------------------------------------------------ */
int gmmvi_device_count(void);
int gmmvi_ctx_create(gmmvi_ctx** out, int device);
void gmmvi_ctx_destroy(gmmvi_ctx* ctx);
const char* gmmvi_last_error(gmmvi_ctx* ctx);          /* ctx may be NULL: last error of a failed create */
int gmmvi_sync(gmmvi_ctx* ctx);
int gmmvi_num_cus(gmmvi_ctx* ctx);                      /* compute units of the context's device: the launch geometries depend on it */
int gmmvi_malloc(gmmvi_ctx* ctx, size_t nbytes, void** out_dev);
int gmmvi_free(gmmvi_ctx* ctx, void* dev);
int gmmvi_upload(gmmvi_ctx* ctx, void* dst_dev, const void* src_host, size_t nbytes);
int gmmvi_download(gmmvi_ctx* ctx, void* dst_host, const void* src_dev, size_t nbytes);   /* synchronises */
int gmmvi_copy(gmmvi_ctx* ctx, void* dst_dev, const void* src_dev, size_t nbytes);
int gmmvi_fill_f32(gmmvi_ctx* ctx, float* dst_dev, float value, size_t count);
/* dst[i, :] = src[idx[i], :] for rows of row_words 4-byte words (fp32 or int32): SampleDB.remove_every_nth_sample /
 * get_random_sample / background-component gather (optimization/sample_db.py:63-79,137-152,222-224 tf.gather). */
int gmmvi_gather_rows(gmmvi_ctx* ctx, const void* src_dev, const int32_t* idx_dev, int n_rows, int row_words,
                      void* dst_dev);
/* Up to 8 device-to-device copies in ONE launch (the per-iteration SampleDB append of samples, target values,
 * gradients and component snapshots, optimization/sample_db.py:115-124; sizes in bytes, multiples of 4). */
int gmmvi_copy_batch(gmmvi_ctx* ctx, int n, void* const* dst_dev, const void* const* src_dev, const size_t* nbytes);
/* De-interleaves an all-gathered buffer: every rank contributed one chunk of chunk_words 4-byte words made of n_seg <= 8
 * consecutive segments (seg_words[j] words each); dst[j] receives segment j of all ranks back to back,
 * dst[j][r * seg_words[j] + i] = src[r * chunk_words + seg_offset_j + i].  One launch; lets the sharded iteration send
 * several arrays in ONE collective (sharded.py E1-E3). */
/* GMM.replace_weights (models/gmm.py:173-181) on the device: out = lw - logsumexp(lw), the sum in fp64. */
int gmmvi_normalize_logw(gmmvi_ctx* ctx, const float* logw_in_dev, int n, float* logw_out_dev);
/* VipsComponentAdaptation.add_at_best_location (component_adaptation.py:192-226): index_out[0] = argmax_n of
 * log p~(x_n) - max(max_m log q(x_m) - threshold, log q(x_n)) over n candidates (first index on ties, fp64). */
int gmmvi_add_heuristic_argmax(gmmvi_ctx* ctx, const float* model_ld_dev, const float* target_lnpdfs_dev, int n, double threshold,
                               int32_t* index_out_dev);
int gmmvi_unpack_gathered(gmmvi_ctx* ctx, const void* src_dev, int n_ranks, size_t chunk_words, int n_seg,
                          const size_t* seg_words, void* const* dst_dev);
/* dst[i * stride] = value, i < count: a new component's column of the [H, Kcap] reward / weight history rings
 * (models/gmm_wrapper.py:121-124). */
int gmmvi_fill_strided_f32(gmmvi_ctx* ctx, float* dst_dev, size_t stride, size_t count, float value);
/* a[r, idx:K-1] = a[r, idx+1:K] for every row r of a [rows, stride] array: GmmWrapper.remove_component's history
 * update (models/gmm_wrapper.py:145-146). */
int gmmvi_remove_column_f32(gmmvi_ctx* ctx, float* a_dev, int rows, size_t stride, int K, int idx);
/* dst[i] = src[i] + value: the mapping offset of SampleDB.add_samples (optimization/sample_db.py:115). */
int gmmvi_add_scalar_i32(gmmvi_ctx* ctx, int32_t* dst_dev, const int32_t* src_dev, int32_t value, size_t count);
/* dst[i] = exp(src[i])  (GMM.weights, models/gmm.py:171; weight history, models/gmm_wrapper.py:182). */
int gmmvi_exp_f32(gmmvi_ctx* ctx, float* dst_dev, const float* src_dev, size_t count);
/* dst[i] = log(exp(a[i] + ca) + exp(b[i] + cb)): joins the two halves of SampleDB's background density when the window grows by
 * one append -- the mixture of the components that were already in the window (known for the old samples from the previous
 * get_newest_samples call) and the mixture of the new components (optimization/sample_db.py:216-227 evaluates the whole
 * window's mixture on all of its samples every time). */
int gmmvi_logaddexp_f32(gmmvi_ctx* ctx, float* dst_dev, const float* a_dev, float ca, const float* b_dev, float cb,
                        size_t count);
/* Per-append partial densities of SampleDB's background mixture: the components of a window are grouped by the append that
 * contributed them (G groups, offsets [G+1] into the component axis); out[g * out_stride + col0 + n] = log sum_{j in group g}
 * exp(logw[j] + ld[j, n]) from the component log densities ld [Kw, N].  The window's density (optimization/sample_db.py:
 * 216-227) is the log-sum-exp of those rows (gmmvi_combine_partials); rows of appends that stay wholly inside the sliding
 * window are kept from one iteration to the next (gmmvi_copy_2d_f32 moves the surviving block). */
int gmmvi_segment_lse_f32(gmmvi_ctx* ctx, int G, const int32_t* offsets_dev, const float* logw_dev, const float* ld_dev, int N,
                          float* out_dev, size_t out_stride, int col0);
/* dst[r * dst_stride + c] = src[r * src_stride + c], r < rows, c < cols. */
int gmmvi_copy_2d_f32(gmmvi_ctx* ctx, float* dst_dev, size_t dst_stride, const float* src_dev, size_t src_stride, int rows,
                      int cols);
/* timing helpers for bench.py: HIP events on the context's stream */
int gmmvi_event_create(gmmvi_ctx* ctx, void** out_event);
int gmmvi_event_destroy(gmmvi_ctx* ctx, void* event);
int gmmvi_event_record(gmmvi_ctx* ctx, void* event);
int gmmvi_event_elapsed_ms(gmmvi_ctx* ctx, void* start, void* stop, float* out_ms);       /* synchronises on stop */
int gmmvi_event_synchronize(gmmvi_ctx* ctx, void* event);                                   /* waits until the stream has reached it */
/* A read-back that does not wait: dst is pinned host memory from gmmvi_host_alloc; valid once an event recorded behind the copy
 * has been reached (the effective sample sizes of the NEXT iteration's reuse window are fetched this way while the current
 * iteration's last launches still run: optimization/fused.py). */
int gmmvi_host_alloc(gmmvi_ctx* ctx, size_t nbytes, void** out_pinned_host);
int gmmvi_host_free(gmmvi_ctx* ctx, void* pinned_host);
int gmmvi_download_async(gmmvi_ctx* ctx, void* dst_pinned_host, const void* src_dev, size_t nbytes);

/* Grow-in-place device buffers (what optimization/sample_db.py keeps its arrays in; the reference's SampleDB concatenates
   tensors, sample_db.py:97-135): reserve an address range once, map physical memory behind its used part in chunks of
   *chunk_bytes_out; growing copies nothing.  gmmvi_vmm_grow: mapped_bytes / new_mapped_bytes are multiples of the chunk size.
   gmmvi_vmm_release waits for the context's stream, unmaps and frees the range. */
int gmmvi_vmm_reserve(gmmvi_ctx* ctx, size_t max_bytes, void** base_out, size_t* chunk_bytes_out);
int gmmvi_vmm_grow(gmmvi_ctx* ctx, void* base, size_t chunk_bytes, size_t mapped_bytes, size_t new_mapped_bytes);
int gmmvi_vmm_release(gmmvi_ctx* ctx, void* base, size_t chunk_bytes, size_t mapped_bytes, size_t reserved_bytes);

/* Per-kernel timing for bench.py's roofline leg: while enabled, every kernel-launching entry point brackets its
 * launches with HIP events on the context's stream.  gmmvi_profile_report synchronises, writes one line per kernel
 * name ("name count total_ms total_pairs\n"; total_pairs = (sample, component) pairs processed, 0 where not counted) into
 * buf and clears the records. */
int gmmvi_profile_enable(gmmvi_ctx* ctx, int on);
int gmmvi_profile_report(gmmvi_ctx* ctx, char* buf, size_t buf_size);

/* ---- component parameter blocks ---------------------------------------------------------------------- */
/* Number of floats of one packed component block for dimension D (D <= 64: padded dimension, reciprocal diagonal,
 * row- and column-packed strict lower triangle of L, log-normaliser, then for padded D <= 24 the "sweep stream" the packed
 * two-samples-per-lane density kernel reads in order -- mean, log-normaliser, the triangle by columns and by rows with the
 * reciprocal diagonal entries in place -- and for padded D >= 32 L^-1 as matrix-core operand fragments;
 * 64 < D <= 512: mu, log-normaliser, dense L^-1).  0 for an unsupported dimension. */
size_t gmmvi_packed_stride(int D);
/* Pack K components (means[K,D], chols[K,D,D] lower-triangular dense) for the density kernels.
 * family/nu select the log-normaliser (Gaussian: full_cov_gmm.py:60-61; Student-t: student_t_mixture.py:40-44).
 * Also writes inv_chols[K,D,D] = L^-1 when inv_chols_dev != NULL (sample_db.py:121 tf.linalg.inv(chols)). */
int gmmvi_pack_components(gmmvi_ctx* ctx, int family, float nu, int K, int D, const float* means_dev,
                          const float* chols_dev, float* packed_dev, float* inv_chols_dev);
/* Batched Cholesky covs[K,D,D] -> chols[K,D,D] (full_cov_gmm.py:23, :64-68); ok[K] = 0 on a non-positive pivot. */
int gmmvi_cholesky(gmmvi_ctx* ctx, int K, int D, const float* covs_dev, float* chols_dev, int32_t* ok_dev);

/* ---- densities ----------------------------------------------------------------------------------------- */
/* For every sample n and component k:  ld[k,n] = log f_k(x_n)  and, over components,
 *   lp[n]   = logsumexp_k(logw[k] + ld[k,n])
 *   grad[n] = sum_k softmax_k(logw[k] + ld[k,n]) * d/dx log f_k(x_n)
 * Replaces FullCovGMM.component_log_densities (models/full_cov_gmm.py:56-62), GMM.log_density /
 * log_densities_also_individual / log_density_and_grad (models/gmm.py:183-216,274-300), SampleDB.evaluate_background
 * (optimization/sample_db.py:154-192, with logw = log(count/N)) and the GMM / Student-t targets with their
 * autodiff gradient (target_distributions/gmm.py:38-40, student_t_mixture.py:66-68, sample_selector.py:74-77).
 * Any of ld_out_dev[K,N], lp_out_dev[N], grad_out_dev[N,D] may be NULL. */
int gmmvi_mixture_eval(gmmvi_ctx* ctx, int family, float nu, int K, int D, const float* packed_dev,
                       const float* logw_dev, const float* X_dev, int N, float* ld_out_dev, float* lp_out_dev,
                       float* grad_out_dev);

/* Same pass with a SECOND set of mixture weights over the same components: lp2[n] = logsumexp_k(logw2[k] + ld[k,n]).
 * Fuses SampleDB.get_newest_samples' background density (weights = sample counts, sample_db.py:221-227) with
 * GMM.log_density_and_grad (models/gmm.py:274-300) when the active samples were drawn from the current components
 * (reuse ratio 0): one sweep over the (sample, component) pairs instead of two. */
int gmmvi_mixture_eval_dual(gmmvi_ctx* ctx, int family, float nu, int K, int D, const float* packed_dev,
                            const float* logw_dev, const float* logw2_dev, const float* X_dev, int N, float* ld_out_dev,
                            float* lp_out_dev, float* grad_out_dev, float* lp2_out_dev);

/* Planar n-link robot target (target_distributions/planar_robot.py:29-66) and its gradient. goals_dev[G,2]. */
int gmmvi_target_planar(gmmvi_ctx* ctx, int D, const float* prior_std_dev, int G, const float* goals_dev,
                        float likelihood_std, const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev);

/* Bayesian logistic regression (target_distributions/logistic_regression.py:20-67) and its analytic gradient.
 * A_dev[M,D] = diag(s) X~ (standardised features behind a bias column, s_m = -1 for label 1, +1 for label 0):
 *   lp[n]   = sum_m log sigmoid(a_m . w_n) + sum_d log N(w_nd; prior_mean, prior_std^2)
 *   grad[n] = sum_m sigmoid(-a_m . w_n) a_m - (w_n - prior_mean) / prior_std^2
 * W_dev[N,D]; grad_out_dev may be NULL.  1 <= D <= GMMVI_MAX_DIM_BLOCKED, M >= 1. */
int gmmvi_target_logreg(gmmvi_ctx* ctx, int D, int M, const float* A_dev, float prior_mean, float prior_std,
                        const float* W_dev, int N, float* lp_out_dev, float* grad_out_dev);

/* The minibatch variant (target_distributions/logistic_regression.py:70-142, LogisticRegression_minibatch) on the T
 * training rows A_dev[T,D] (signed, as above).  Within call `call` the rows are permuted by rho (the Feistel/Philox
 * permutation of DESIGN.md 6 keyed by seed, counter (R | i << 24, 0, call, 4): stream id 4) and sample n takes the batch
 * b = n mod nb of B rows, row(n, j) = rho(b B + j):
 *   lp[n]   = (T/B) sum_j log sigmoid(a_row(n,j) . w_n) + sum_d log N(w_nd; prior_mean, prior_std^2)
 *   grad[n] = (T/B) sum_j sigmoid(-a_row(n,j) . w_n) a_row(n,j) - (w_n - prior_mean) / prior_std^2
 * W_dev[N,D]; grad_out_dev may be NULL; N == 0 launches nothing.  1 <= D <= 128, 1 <= B <= T, nb >= 1, nb B <= T,
 * prior_std > 0; anything else: GMMVI_ERR_ARG.  Bitwise reproducible for a given (seed, call). */
int gmmvi_target_logreg_mb(gmmvi_ctx* ctx, int D, int T, const float* A_dev, int B, int nb, uint64_t seed, uint32_t call,
                           float prior_mean, float prior_std, const float* W_dev, int N, float* lp_out_dev,
                           float* grad_out_dev);

/* Bayesian-neural-network regression (target_distributions/bnn.py:59-311,385-448, the WINE posterior) and its analytic
 * gradient.  Network F -> H1 -> H2 -> 1 (sigmoid, sigmoid, linear); W_dev[N,D] in the reference's layout W1 [F,H1]
 * row-major, b1 [H1], W2 [H1,H2], b2 [H2], W3 [H2], b3, so D = F H1 + H1 + H1 H2 + H2 + H2 + 1.  X_dev[T,F], y_dev[T]:
 * the training set.  Sample n sees the B rows pi_{seed,call,e}(p mod T), p = n B + j, e = p div T (the Feistel/Philox
 * minibatch stream of csrc/bnn.hip, stream id 3):
 *   lp[n]   = likelihood_scaling (-(T/B) sum_j (y - f(x; w_n))^2 - 0.5 sum_d w_nd^2 / prior_std^2)
 *   grad[n] = d lp[n] / d w_n
 * grad_out_dev may be NULL.  1 <= F <= 32, 1 <= H1, H2 <= 16, 1 <= B <= T; anything else: GMMVI_ERR_ARG. */
int gmmvi_target_bnn(gmmvi_ctx* ctx, int F, int H1, int H2, int T, const float* X_dev, const float* y_dev, uint64_t seed,
                     uint32_t call, int B, float likelihood_scaling, float prior_std, const float* W_dev, int N,
                     float* lp_out_dev, float* grad_out_dev);

/* The same network's outputs, forward only: out[s, m] = f(X[m]; W[s]).  W_dev[S,D], X_dev[M,F], S <= 65535. */
int gmmvi_bnn_predict(gmmvi_ctx* ctx, int F, int H1, int H2, const float* W_dev, int S, const float* X_dev, int M,
                      float* out_dev);

/* Bayesian-neural-network classification (target_distributions/bnn.py, BNN_LNPDF with the network and loss of BNN_MNIST)
 * and its analytic gradient.  Network F -> H (ReLU) -> C (logits); W_dev[N,D] in the reference's layout W1 [F,H] row-major,
 * b1 [H], W2 [H,C] row-major, b2 [C], so D = F H + H + H C + C.  X_dev[T,F] f32, labels_dev[T] int32 in [0, C): the
 * training set.  Sample n sees the B rows of gmmvi_target_bnn's minibatch stream (stream id 3) for (seed, call):
 *   lp[n]   = likelihood_scaling (-(T/B) sum_j (logsumexp(l_j) - l_j[y_j]) - 0.5 sum_d w_nd^2 / prior_std^2)
 *   grad[n] = d lp[n] / d w_n      (ReLU derivative 1 where the pre-activation is positive, else 0)
 * grad_out_dev may be NULL (lp is bitwise the same); N == 0 launches nothing.  1 <= F <= 1024, 1 <= H <= 128,
 * 2 <= C <= 16, 1 <= B <= min(T, 1024), prior_std > 0; anything else: GMMVI_ERR_ARG.  A label outside [0, C) selects no
 * logit (the caller checks the labels).  Bitwise reproducible for a given (seed, call): no atomics. */
int gmmvi_target_bnn_classifier(gmmvi_ctx* ctx, int F, int H, int C, int T, const float* X_dev, const int32_t* labels_dev,
                                uint64_t seed, uint32_t call, int B, float likelihood_scaling, float prior_std,
                                const float* W_dev, int N, float* lp_out_dev, float* grad_out_dev);

/* The same network's logits, forward only: logits[s, m, c] of X[m] under W[s].  W_dev[S,D], X_dev[M,F],
 * logits_out_dev[S,M,C]; S <= 65535; S == 0 or M == 0 launches nothing. */
int gmmvi_bnn_classifier_predict(gmmvi_ctx* ctx, int F, int H, int C, const float* W_dev, int S, const float* X_dev, int M,
                                 float* logits_out_dev);

/* Generic Bayesian-neural-network posterior (target_distributions/bnn.py, BNN_LNPDF: any hidden_units list, one activation
 * per layer, MSE or sparse categorical cross-entropy from logits) and its analytic gradient (csrc/bnn_mlp.hip).
 * The network has n_layers dense layers, widths[0] = F inputs, widths[1 .. n_layers - 1] hidden units and widths[n_layers]
 * outputs; W_dev[N,D] in the reference's layout, per layer W [in, out] row-major, then b [out].  loss 0: MSE, one output,
 * y_dev[T] f32; loss 1: cross-entropy from logits, C = widths[n_layers] classes, y_dev[T] int32 in [0, C).  Sample n sees
 * the B rows of gmmvi_target_bnn's minibatch stream (stream id 3) for (seed, call):
 *   lp[n]   = likelihood_scaling (-(T/B) sum_j loss_j - 0.5 sum_d w_nd^2 / prior_std^2)
 *   grad[n] = d lp[n] / d w_n      (ReLU derivative 1 where the pre-activation is positive, else 0)
 * grad_out_dev may be NULL (lp is bitwise the same); N == 0 launches nothing.  2 <= n_layers <= 4, 1 <= F <= 1024, every
 * hidden width in 1 .. 128 (the same cap for every hidden layer), 2 <= C <= 16, the output layer linear,
 * 1 <= B <= min(T, 1024), D <= GMMVI_MAX_DIM_DIAG, prior_std > 0; anything else: GMMVI_ERR_ARG, and gmmvi_last_error names
 * the limit.  A label outside [0, C) selects no logit.  Bitwise reproducible for a given (seed, call): no atomics. */
#define GMMVI_MLP_MAX_LAYERS 4
enum { GMMVI_MLP_LINEAR = 0, GMMVI_MLP_SIGMOID = 1, GMMVI_MLP_RELU = 2, GMMVI_MLP_TANH = 3 };
enum { GMMVI_MLP_LOSS_MSE = 0, GMMVI_MLP_LOSS_CROSS_ENTROPY = 1 };
typedef struct gmmvi_mlp_desc {
    int32_t n_layers;                               /* dense layers, 2 .. 4 (one to three hidden layers) */
    int32_t widths[GMMVI_MLP_MAX_LAYERS + 1];       /* F, the hidden widths, the output width */
    int32_t activations[GMMVI_MLP_MAX_LAYERS];      /* one per layer: GMMVI_MLP_LINEAR / SIGMOID / RELU / TANH */
    int32_t loss;                                   /* GMMVI_MLP_LOSS_MSE / GMMVI_MLP_LOSS_CROSS_ENTROPY */
} gmmvi_mlp_desc;
int gmmvi_target_mlp(gmmvi_ctx* ctx, const gmmvi_mlp_desc* net, int T, const float* X_dev, const void* y_dev, uint64_t seed,
                     uint32_t call, int B, float likelihood_scaling, float prior_std, const float* W_dev, int N,
                     float* lp_out_dev, float* grad_out_dev);

/* The same network's outputs, forward only: out[s, m] (MSE) or logits[s, m, c] (cross-entropy) of X[m] under W[s].
 * W_dev[S,D], X_dev[M,F]; S <= 65535; S == 0 or M == 0 launches nothing. */
int gmmvi_mlp_predict(gmmvi_ctx* ctx, const gmmvi_mlp_desc* net, const float* W_dev, int S, const float* X_dev, int M,
                      float* out_dev);

/* Talos humanoid inverse kinematics (target_distributions/talos_ik.py; DESIGN.md 6, "Talos (defined, not reproduced)") and
 * its analytic gradient.  model_dev: the packed f32 table of talos_ik.TalosModel (28 revolute joints, 4 tips, lumped
 * masses); context_dev[3]: the left gripper's goal.  X_dev[N,34] = [q (28), p_b (3), roll, pitch, yaw]:
 *   lp[n]   = joint limits + centre of mass over the left foot + right foot + left foot + left gripper (the five terms)
 *   grad[n] = d lp[n] / d x_n (geometric Jacobian)
 * grad_out_dev may be NULL; N == 0 launches nothing.  One lane per sample, no atomics: bitwise reproducible. */
int gmmvi_target_talos(gmmvi_ctx* ctx, const float* model_dev, const float* context_dev, const float* X_dev, int N,
                       float* lp_out_dev, float* grad_out_dev);

/* The forward kinematics of the same model: poses_out_dev[N,4,12] = per tip (r_gripper, l_gripper, r_foot, l_foot) the
 * world position (3) and rotation (9, row-major); com_out_dev[N,3] the world centre of mass of the 37 path links. */
int gmmvi_talos_fk(gmmvi_ctx* ctx, const float* model_dev, const float* X_dev, int N, float* poses_out_dev, float* com_out_dev);

/* ---- user-defined device targets -------------------------------------------------------------------------------------------
 * The counterpart of subclassing LNPDF (target_distributions/lnpdf.py, examples/4_gmmvi_runner_with_custom_environments.py)
 * at device speed: the target is HIP source text, compiled at run time (hiprtc, loaded on first use; without libhiprtc.so the
 * calls below return GMMVI_ERR_HIP and name it) for the device of the context and evaluated by wrapper kernels of this
 * library (csrc/custom_target_wrap.inc).  The contract: the source defines exactly one function
 *
 *     __device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad);
 *
 *   - x: the sample's row of D floats; params: the target's own device array (params_dev below; NULL when it has none);
 *   - grad: NULL, or the sample's gradient row.  With grad == NULL the function returns the log density and writes nothing;
 *     with a row it also writes ALL D entries of the gradient of the log density;
 *   - the function is pure per sample: no barriers, no LDS of its own, no atomics, no writes other than grad[0 .. D);
 *   - it may define helper __device__ functions and constants beside it; the text is compiled with -O3 -std=c++17, without
 *     fast-math, and may not define names that begin with gmmvi_ other than gmmvi_user_target.
 * A function that breaks the contract (reads or writes out of bounds, synchronises, never returns) can fault or hang the
 * device, like any kernel: the library cannot check it.
 * Two routes evaluate it.  Staged (D <= GMMVI_CUSTOM_STAGED_MAX_DIM): a wavefront copies 64 consecutive rows of X into LDS,
 * every lane calls the function on its LDS row with an LDS gradient row, and the gradient tile is written back as one
 * coalesced stream.  Direct (D <= GMMVI_MAX_DIM_DIAG): the lane is the sample, x and grad are the global rows. */
#define GMMVI_CUSTOM_STAGED_MAX_DIM 120   /* two [64][D | 1] fp32 images: 61952 B of LDS at D = 120 */
typedef struct gmmvi_custom_target gmmvi_custom_target;
/* Compiles source + wrapper kernels for `arch` ("gfx950") and discards the code object.  Needs no device and no context.
 * log_out[log_cap] (may be NULL) receives the compiler log, cut to fit.  0; GMMVI_ERR_ARG: the source does not compile (a
 * source without gmmvi_user_target: the log names it); the text is also in gmmvi_last_error(NULL). */
int gmmvi_custom_target_check(const char* source, const char* arch, char* log_out, size_t log_cap);
/* Compiles for the context's device (--offload-arch=<its gcnArchName>) and loads the code object.  The context keeps its loaded
 * targets keyed by a hash of the source: the same source again returns the same handle (counted; one release per compile).
 * A compile error: GMMVI_ERR_ARG, the compiler log in gmmvi_last_error.  Everything left is released with the context. */
int gmmvi_custom_target_compile(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out);
int gmmvi_custom_target_release(gmmvi_ctx* ctx, gmmvi_custom_target* target);    /* waits for the stream; NULL is a no-op */
/* lp[n] = gmmvi_user_target(X[n], D, params, grad ? grad[n] : NULL).  X_dev[N,D], lp_out_dev[N], grad_out_dev[N,D] or NULL
 * (values only).  route: 0 auto (staged up to GMMVI_CUSTOM_STAGED_MAX_DIM, direct above), 1 staged, 2 direct.  N >= 1,
 * 1 <= D <= GMMVI_MAX_DIM_DIAG, route 1 with D above the cap, a NULL X / lp / handle, a handle of another context: GMMVI_ERR_ARG
 * before any launch. */
int gmmvi_target_custom(gmmvi_ctx* ctx, const gmmvi_custom_target* target, int D, const float* params_dev,
                        const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int route);

/* ---- differentiated user-defined targets: density in, gradient out -------------------------------------------------------------
 * The counterpart of upstream's GradientTape over a user's log_density (SampleSelector.get_target_grads): the source defines the
 * log density only, as a template,
 *
 *     template <class T, class X>
 *     __device__ T gmmvi_user_density(X x, int D, const float* params);
 *
 *   - x[i] yields a T for 0 <= i < D; params: the target's own device array, or NULL; the function returns the log density;
 *   - it is pure per sample under the rules of gmmvi_user_target above: no barriers, no LDS, no atomics, no writes to memory
 *     that is not its own locals; the same flags; no names that begin with gmmvi_ other than gmmvi_user_density;
 *   - for a value call the library instantiates T = float, X = const float*;
 *   - for a gradient call T is the library's dual number, a value and GMMVI_CUSTOM_AUTODIFF_TANGENTS tangents, and X is a view
 *     that returns {x[i], e_(i - first)} on read: the seeded input is never stored per lane.
 * The library puts its dual-number text (csrc/custom_target_autodiff.inc) and then the wrapper kernels behind the source; the
 * source stays first, so the compiler's line numbers are the user's, and the overloads are found by argument-dependent lookup
 * when the template is instantiated (one declaration, gmmvi_value(float), goes in front of the source's first line, on that
 * line: a float has no namespace for that lookup).  In this mode and in the data mode below, not in the hand-written one, the
 * compiler is also given -DGMMVI_CUSTOM_AUTODIFF_TANGENTS=<W>, so a text can tell the modes apart.  On a T the text defines
 *   - + - * / and += -= *= /= between T and T, T and float, float and T; unary minus;
 *   - < <= > >= == !=, decided on the values;
 *   - exp expm1 log log1p sqrt rsqrt sin cos tan tanh atan fabs fmax fmin, pow(T, float) and pow(T, T), each also under its
 *     f-suffixed name (expf, ...);
 *   - lgamma, and erf erfc, these two also under their f-suffixed names: the values are ROCm's lgammaf, erff and erfcf, the
 *     derivatives gmmvi_digamma(a) and +-2 / sqrt(pi) exp(-a^2).  lgammaf itself stays a float function: on a T it is a
 *     compile error, spell it lgamma;
 *   - sinh cosh asin acos, each also under its f-suffixed name: the values are ROCm's, the derivatives cosh, sinh and
 *     +-1 / sqrt(1 - a^2), which is infinite at |a| = 1 and NaN beyond;
 *   - gmmvi_digamma(t), gmmvi_sigmoid(t), gmmvi_softplus(t), gmmvi_log_sigmoid(t), and gmmvi_logaddexp between T and T, T and
 *     float, float and T (below);
 *   - gmmvi_erfcx(t), gmmvi_ndtr(t), gmmvi_log_ndtr(t) (below);
 *   - gmmvi_value(t): the float value of a float and of a dual.
 * A float converts to a T (a constant: all tangents 0); a T does not convert to float, so a function outside this list, such
 * as tgammaf, erfinvf or lgammaf, on a T is a compile error (GMMVI_ERR_ARG with the compiler log, as for any source).
 * The library's float functions (csrc/custom_target_special.inc; plain C++, host and device).  In every mode, the hand-written
 * one included, they are declared in front of the source's first line, on that line (where that line begins with a directive, on
 * a line of their own, followed by a line directive that keeps the numbers the user's), and defined behind the source; a source
 * may call them on a float, and must not define these or any other gmmvi_ name:
 *   - float gmmvi_digamma(float x): psi(x) for x > 0, by the recurrence up to x >= 6 and the asymptotic series; x <= 0 and NaN
 *     give NaN (no reflection formula);
 *   - float gmmvi_trigamma(float x): psi'(x), the same way and with the same domain.  It takes a float only: there are no
 *     second derivatives, so gmmvi_trigamma of a T is a compile error;
 *   - float gmmvi_sigmoid(float x): 1 / (1 + e^-x), from e^-|x| alone: exactly 1 and 0 beyond the range of expf;
 *   - float gmmvi_softplus(float x): log(1 + e^x) = fmax(x, 0) + log1p(exp(-|x|));
 *   - float gmmvi_log_sigmoid(float x): -gmmvi_softplus(-x);
 *   - float gmmvi_logaddexp(float a, float b): log(e^a + e^b) = max + log1p(exp(-|a - b|)); a == b, equal infinities
 *     included, gives a + ln 2 and no NaN;
 *   - float gmmvi_erfcx(float x): e^(x^2) erfc(x), from a polynomial of its own and expf, not from erfcf.  Finite and positive
 *     for every finite x >= 0 (1 / (x sqrt(pi)) where x^2 overflows); +inf where 2 e^(x^2) overflows (x < -9.38); NaN for NaN;
 *   - float gmmvi_ndtr(float x): the normal distribution function Phi(x) = erfc(-x / sqrt(2)) / 2, as erfcx(|x| / sqrt(2))
 *     e^(-x^2 / 2) / 2 or one minus that: exactly 0 or 1 only where fp32 has nothing closer;
 *   - float gmmvi_log_ndtr(float x): log Phi(x); for x < 0 log(erfcx(-x / sqrt(2)) / 2) - x^2 / 2, finite for every finite x whose
 *     x^2 / 2 is finite and -inf beyond and at -inf; for x >= 0 log1p(-(1 - Phi(x))), exactly 0 at +inf; NaN for NaN.  It never
 *     takes the logarithm of an underflowed erfcf: log(0.5f * erfcf(-x * 0.70710678f)) is -inf from x = -14.2 on.
 * On a T: gmmvi_erfcx has the derivative 2 a erfcx(a) - 2 / sqrt(pi) (for a >= 0 from a polynomial of its own, the difference
 * cancels; -inf, never NaN, where the value has overflowed); gmmvi_ndtr phi(a) = e^(-a^2 / 2) / sqrt(2 pi) with the rounding of
 * a^2 carried along; gmmvi_log_ndtr phi(a) / Phi(a), for a < 0 as sqrt(2 / pi) / erfcx(-a / sqrt(2)): finite and positive for
 * every finite a at which phi is not below fp32's range, 0 at +inf.  gmmvi_digamma has the derivative gmmvi_trigamma(a); gmmvi_sigmoid s * sigmoid(-a) (not s (1 - s), which cancels for
 * large a); gmmvi_softplus sigmoid(a); gmmvi_log_sigmoid sigmoid(-a); gmmvi_logaddexp sigmoid(a - b) and sigmoid(b - a).
 * Tie rules: fabs has tangent 0 at +-0; fmax and fmin take the first operand's tangent on a tie; a branch on a comparison
 * differentiates the branch taken.  pow(T, T) takes no part of ln(a) in a direction in which the exponent does not move;
 * sqrt, rsqrt and log at 0 have the infinite derivatives of IEEE arithmetic.  lgamma of a T has a NaN derivative at a <= 0
 * (digamma's; the value is still lgammaf's); gmmvi_logaddexp has the derivatives exactly 1/2 and 1/2 on a tie; gmmvi_sigmoid
 * beyond the range of expf is exactly 1 or 0 with derivative exactly 0.
 * Vector primitives on the input view x (csrc/custom_target_vector.inc; declared and defined with the float functions above, in
 * every mode).  X is whatever the mode passes as x: const float* on value calls and in the hand-written mode, the seeded view
 * of this mode, the input view of the tape modes below; each returns that mode's number (float, dual, tape node):
 *   - gmmvi_dot(X x, int first, const float* c, int n):         sum over i < n of c[i] * x[first + i];
 *   - gmmvi_sqdist(X x, int first, const float* c, int n):      sum over i < n of (x[first + i] - c[i])^2;
 *   - gmmvi_sumsq(X x, int first, int n, float center):         sum over i < n of (x[first + i] - center)^2.
 * n <= 0 gives the constant 0: zero tangents, no record.  0 <= first and first + n <= D are the caller's duty, like the index of
 * x[i]: the library cannot check them.  c must stay readable and unchanged until the kernel ends: it may point into row, params
 * or a static table, not into an array local to the user's function, because the reverse sweep reads c after that function has
 * returned; the rule holds in every mode, so that one text serves all of them.  The value comes from one function per primitive
 * for all three number types, so a value call and a gradient call give the same bits.  Its order: four partial sums, element i
 * into partial i mod 4 by one fused multiply-add (fmaf(c[i], x[i], s), fmaf(d, d, s) with d = x[first + i] - c[i] or - center),
 * i ascending, then (s0 + s1) + (s2 + s3).  The derivatives are closed forms: c[k], 2 (x - c[k]), 2 (x - center) by
 * x[first + k], nothing by c.  Forward mode: the tangents of a pass are 16 loads, there is no loop over n with tangents.  Tape
 * modes: one record per call whatever n is (below).
 * Two primitives take an array of T, the number type of the mode (float on value calls and in the hand-written mode, the dual,
 * the tape node); the overloads of the gradient modes are found by argument-dependent lookup on the array's element type:
 *   - gmmvi_wdot(X x, int first, const T* h, int n):            sum over i < n of h[i] * x[first + i];
 *   - gmmvi_logsumexp(const T* a, int n):                       log of the sum over i < n of exp(a[i]).
 * gmmvi_wdot: entries of h may be constants; n <= 0 gives the constant 0 (zero tangents, no record); 0 <= first and
 * first + n <= D are the caller's duty.  The value has the order of gmmvi_dot (fmaf(h[i].value, x[first + i], s), four partial
 * sums), from one function for all three number types: a value call and a gradient call agree bit for bit, and on floats the
 * result has the bits of gmmvi_dot(x, first, h, n).  THERE IS NO LIFETIME RULE FOR h (or for a): unlike c of gmmvi_dot, what
 * the reverse sweep needs is copied into the record, so an array local to the user's function is the normal case.  A const
 * float* in the place of x does not compile in the gradient modes.
 * gmmvi_logsumexp: m = the maximum by fmaxf, i ascending from -inf; s = the sum of expf(a[i] - m) in four partial sums by plain
 * adds, element i into partial i mod 4, merged (s0 + s1) + (s2 + s3); the result is m + logf(s), again from one function for
 * all three number types.  The partials p_i = expf(a[i] - m) / s come from one helper in both gradient modes.  m == -inf (n <= 0
 * or every entry -inf) gives the constant -inf: zero tangents, no record.  If every a[i] is a constant the result is a constant.
 * Any other non-finite maximum is outside the contract and cannot fault (no index depends on a value); what it yields: a +inf
 * entry makes the value and every partial NaN; a NaN entry beside finite ones is dropped from the maximum and makes the value
 * and every partial NaN through s; an array of NaNs alone has m == -inf and gives the constant -inf.
 * Forward mode: tangent j of gmmvi_wdot is the sum over i of x[first + i] * h[i].d[j], by fmaf, i ascending, plus h[k].v for
 * k = x.first + j - first where 0 <= k < n; tangent j of gmmvi_logsumexp is the sum over i of p_i * a[i].d[j], by fmaf.  One
 * pass over n per call.  Tape modes: one node-array record per call, 1 + ceil(n / 2) slots (below).
 * A whole affine layer, a matrix of inputs times an array of T plus a bias, is one call with strides:
 *   - gmmvi_affine(X x, int w, int si, int sj, int b, int sb, const T* h, int n, T* out, int m):
 *         out[j] = (sum over i < n of h[i] * x[w + i * si + j * sj]) + x[b + j * sb]      for j < m.
 * b < 0: no bias term.  A second overload takes const float* h, constants, for example the features of a data row in the first
 * layer; in float code (value calls, the hand-written mode) the two coincide.  out must not alias h.  si >= 1, sj >= 1 (and
 * sb >= 1 with a bias), every index inside [0, D), and distinct (i, j) giving distinct indices are the caller's duty.  Blocks
 * [weights | bias] per unit are si = 1, sj = n + 1, b = w + n, sb = n + 1; W [in, out] row-major and then b [out], the layout of
 * gmmvi_target_bnn below, is si = m, sj = 1, b = w + n * m, sb = 1.  m <= 0 writes nothing; n <= 0: out[j] is the input
 * x[b + j * sb] itself (derivative 1), or the constant 0 without a bias; neither makes a record.  Entries of h may be constants.
 * The value: the sum in the order of gmmvi_wdot (four partial sums, fmaf(h[i].value, x[..], s), element i into partial i mod 4,
 * (s0 + s1) + (s2 + s3)), then the bias by one plain add, from one function for all three number types: a value call and a
 * gradient call agree bit for bit, and with si == 1 out[j] has the bits of gmmvi_wdot(x, w + j * sj, h, n) + x[b + j * sb].
 * There is no lifetime rule for h or out.  A const float* in the place of x does not compile in the gradient modes.
 * Forward mode: one pass over n * m; tangent t of out[j] is the sum over i of x[w + i * si + j * sj] * h[i].d[t] by fmaf, i
 * ascending, then h[i].v where the seeded input x[x.first + t] is the weight (i, j), then 1 where it is the bias of j.  Tape
 * modes: one record group of ceil(n / 2) + 2 + m slots per call (below), where m gmmvi_wdot calls and m adds take
 * m (2 + ceil(n / 2)).
 * The gradient takes ceil(D / W) passes of the dual instantiation, W = GMMVI_CUSTOM_AUTODIFF_TANGENTS, pass `first` writing
 * grad[first + j] for first + j < D; the value is that of the first pass.  That is ceil(D / W) * (1 + W) value evaluations per
 * sample, so a gradient call through such a handle is capped at GMMVI_CUSTOM_AUTODIFF_MAX_DIM; a value call is not. */
#define GMMVI_CUSTOM_AUTODIFF_TANGENTS 16
#define GMMVI_CUSTOM_AUTODIFF_MAX_DIM 512  /* the largest full-covariance dimension */
/* gmmvi_custom_target_check / _compile for a source that defines gmmvi_user_density (a source without it: GMMVI_ERR_ARG, the
 * log names it).  The handle is an ordinary gmmvi_custom_target: gmmvi_target_custom launches it (a gradient pointer with
 * D > GMMVI_CUSTOM_AUTODIFF_MAX_DIM: GMMVI_ERR_ARG before any launch), target kind 5 takes it, gmmvi_custom_target_release
 * releases it.  The mode is part of the context's key: the same text compiled both ways gives two handles. */
int gmmvi_custom_target_check_autodiff(const char* source, const char* arch, char* log_out, size_t log_cap);
int gmmvi_custom_target_compile_autodiff(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out);
/* One operation of the dual-number text on the host (no device, no context): operands {a, da} and {b, db} (a float operand
 * of the operation ignores its tangent, a unary operation ignores b), *value and *tangent receive the result.  op indexes the
 * operations in the order of csrc/autodiff_probe.hip (gmmvi_amd/_lib.py AUTODIFF_OPS names them); comparisons give 1 or 0
 * with tangent 0.  An unknown op or a NULL output: GMMVI_ERR_ARG. */
int gmmvi_autodiff_probe(int op, float a, float da, float b, float db, float* value, float* tangent);
/* The same for the special functions, a list of their own (gmmvi_amd/_lib.py SPECIAL_OPS names them in index order): lgamma;
 * erf and erfc, each under both spellings; gmmvi_digamma, gmmvi_sigmoid, gmmvi_softplus, gmmvi_log_sigmoid, gmmvi_logaddexp in its
 * three operand forms, and gmmvi_trigamma of the float a (a constant: tangent 0). */
int gmmvi_autodiff_probe_special(int op, float a, float da, float b, float db, float* value, float* tangent);
/* A second list, of one-operand functions (gmmvi_amd/_lib.py EXTRA_OPS names them in index order): gmmvi_erfcx, gmmvi_ndtr,
 * gmmvi_log_ndtr; sinh, cosh, asin and acos, each under both spellings. */
int gmmvi_autodiff_probe_extra(int op, float a, float da, float* value, float* tangent);
/* One vector primitive on host arrays, in the pass seeded at seed_first (gmmvi_amd/_lib.py VECTOR_OPS names the operations in
 * index order: gmmvi_dot, gmmvi_sqdist, gmmvi_sumsq): x[D], c[n] (unused by gmmvi_sumsq, as center is by the other two);
 * *value and tangents[GMMVI_CUSTOM_AUTODIFF_TANGENTS], tangents[j] the derivative by x[seed_first + j].  An unknown op, a NULL
 * array, D < 1, first < 0, seed_first < 0 or first + n > D: GMMVI_ERR_ARG. */
int gmmvi_autodiff_probe_vector(int op, const float* x, int D, int first, int n, const float* c, float center, int seed_first,
                                float* value, float* tangents);
/* One primitive on an array of duals, in the pass seeded at seed_first (gmmvi_amd/_lib.py NODE_OPS names the operations in
 * index order: gmmvi_wdot, gmmvi_logsumexp).  The array is h[i] = tanh(x[src + i]) for i < n; where every > 0 and
 * i % every == every - 1 the entry is the constant tanhf(x[src + i]) instead (every = 1: all constants).  The call is
 * gmmvi_wdot(x, first, h, n) or gmmvi_logsumexp(h, n); *value and tangents[GMMVI_CUSTOM_AUTODIFF_TANGENTS] as above.  An
 * unknown op, a NULL array, D < 1, n > 64, src + n > D, first + n > D or a negative argument: GMMVI_ERR_ARG. */
int gmmvi_autodiff_probe_nodes(int op, const float* x, int D, int first, int n, int src, int every, int seed_first, float* value,
                               float* tangents);
/* The same call on an array whose entries are the inputs themselves, h[i] = x[src + i], which may be -inf: the tangents of
 * gmmvi_logsumexp are then its partials p_i bit for bit.  The same arguments are GMMVI_ERR_ARG. */
int gmmvi_autodiff_probe_nodes_inputs(int op, const float* x, int D, int first, int n, int src, int seed_first, float* value,
                                      float* tangents);
/* One gmmvi_affine(x, w, si, sj, b, sb, h, n, out, m) in the pass seeded at seed_first.  The array is that of
 * gmmvi_autodiff_probe_nodes (h[i] = tanh(x[src + i]), every `every`-th entry a constant); inputs != 0: h[i] = x[src + i], the
 * inputs themselves; floats != 0: the same values as a const float*, the overload that takes constants.  values[m] receives
 * out[0 .. m).  The output is out[pick] for pick >= 0 and gmmvi_logsumexp(out, m), which consumes every output, for pick == -1
 * (the constant 0 for m == 0): *value and tangents[GMMVI_CUSTOM_AUTODIFF_TANGENTS] are its value and derivatives by
 * x[seed_first + t].  A NULL array, D < 1, n or m outside [0, 64], si < 1, sj < 1, sb < 1 with a bias, a negative w, src, every
 * or seed_first, src + n > D, a weight or bias index outside [0, D), or pick outside [-1, max(m, 1)): GMMVI_ERR_ARG.  Distinct
 * (i, j) with distinct indices stay the caller's duty. */
int gmmvi_autodiff_probe_affine(const float* x, int D, int w, int si, int sj, int b, int sb, int n, int m, int src, int every,
                                int inputs, int floats, int pick, int seed_first, float* values, float* value, float* tangents);

/* ---- user-defined targets summed over a data set --------------------------------------------------------------------------------
 * Posteriors of the shape  log p(x) = log prior(x) + sum over the data rows r of log p(data_r | x):  the source defines one
 * row's term and the prior, value-only templates under the purity rules and with the operations of gmmvi_user_density above,
 *
 *     template <class T, class X> __device__ T gmmvi_user_row  (X x, int D, const float* row, int C, const float* params);
 *     template <class T, class X> __device__ T gmmvi_user_prior(X x, int D, const float* params);
 *
 *   - row: the C floats of one data row (plain float, never differentiated); params: the target's own device array, or NULL;
 *   - the text may not define names that begin with gmmvi_ other than these two (and gmmvi_user_density / gmmvi_user_target
 *     behind a test of the mode's macros: this mode defines GMMVI_CUSTOM_AUTODIFF_TANGENTS and GMMVI_AD_NO_ADAPTER).
 * The target is
 *
 *     lp(x) = prior(x) + s * sum_{r in R} row(x, data[r])
 *
 *   - full data (minibatch == 0): R = all T rows in index order, s = 1;
 *   - a minibatch of B rows for (seed, call) (minibatch == 1): R = { pi(j) : 0 <= j < B } in the order of j, with
 *     pi(j) = gmmvi_feistel_permute(j, epoch 0, call, stream 5, T, h, seed lo, seed hi) (csrc/feistel.h; NumPy:
 *     minibatch_stream.data_minibatch_rows) and s = (float)T / (float)B.  One batch per call, shared by all samples (upstream's
 *     use_own_batch_per_sample=False); B == T is a permuted full pass.
 * Order of the arithmetic, all fp32: the row terms are added first (order below); s multiplies the merged row sum ONCE; the
 * prior is added last.  The gradient is the same expression on dual numbers: s * (sum of the row tangents) + prior tangent.
 * Kernels (csrc/custom_target_data.inc): a workgroup of 256 threads = 4 waves serves 64 consecutive samples, lane = sample in
 * every wave; the grid is ceil(N / 64) x chunks.  A workgroup owns one contiguous chunk of rows_per_chunk positions of the row
 * list, its wave w the positions w, w + 4, ... of the chunk; the row index (and the Feistel walk behind it) is wave-uniform, so
 * the row's floats come through uniform loads.  x is staged in LDS up to GMMVI_CUSTOM_STAGED_MAX_DIM and read from global memory
 * above.  A value call is one float instantiation per (sample, row); a gradient call makes ceil(D / W) passes of the dual
 * instantiation, W = GMMVI_CUSTOM_AUTODIFF_TANGENTS, the value taken from pass 0, and is capped at GMMVI_CUSTOM_AUTODIFF_MAX_DIM.
 * Summation order (no atomics; the same inputs and the same chunk count give the same bits): a wave adds its rows in position
 * order; wave 0 adds the sums of waves 1, 2, 3 in that order; with more than one chunk the partials [chunks][N] and
 * [chunks][N][D] go to the context's scratch and a second kernel adds them in chunk order.  Different chunk counts round
 * differently: results agree within the rounding of the sum, not bitwise. */
int gmmvi_custom_target_check_data(const char* source, const char* arch, char* log_out, size_t log_cap);
/* A source without gmmvi_user_row or without gmmvi_user_prior: GMMVI_ERR_ARG, the log names the missing one.  The handle is an
 * ordinary gmmvi_custom_target (released by gmmvi_custom_target_release; the mode is part of the context's key), launched by
 * gmmvi_target_custom_data only: gmmvi_target_custom, and so target kind 5, refuse it with GMMVI_ERR_ARG. */
int gmmvi_custom_target_compile_data(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out);
/* The launch plan, a host function (no device, no context).  chunks_requested == 0 (auto): enough chunks that
 * ceil(N / 64) * chunks workgroups reach 256 (one per compute unit of an MI355X), but at most rows / 32, so that every wave of
 * a chunk has at least 8 rows; at least 1.  chunks_requested > 0 is honoured up to one row per chunk (and 65535).  Then
 * *rows_per_chunk = ceil(rows / chunks) and *chunks = ceil(rows / *rows_per_chunk): the last chunk is never empty.  N < 1,
 * rows outside 1 .. 2^31 - 1, a negative request or a NULL output: GMMVI_ERR_ARG. */
int gmmvi_custom_data_plan(int N, int64_t rows, int chunks_requested, int* chunks, int* rows_per_chunk);
/* lp[n] (and grad[n] when grad_out_dev != NULL) of the target above.  data_dev[T,C] fp32, X_dev[N,D], lp_out_dev[N],
 * grad_out_dev[N,D] or NULL.  minibatch: 0 full data in index order, 1 the batch of (seed, call); the flag, not B, chooses.
 * chunks_requested as for gmmvi_custom_data_plan with rows = T (full data) or B.  GMMVI_ERR_ARG before any launch, naming the
 * limit: T outside 1 .. 2^31 - 1; C < 1; B outside 1 .. T (in either mode; pass B = T with full data); N < 1; D outside
 * 1 .. GMMVI_MAX_DIM_DIAG; a gradient pointer with D > GMMVI_CUSTOM_AUTODIFF_MAX_DIM (a value call runs above); a NULL data_dev,
 * X_dev or lp_out_dev; a handle of another mode or context.  Profiling tags: target_custom_data, target_custom_data_merge. */
int gmmvi_target_custom_data(gmmvi_ctx* ctx, const gmmvi_custom_target* target, int D, const float* params_dev,
                             const float* data_dev, int64_t T, int C, int minibatch, int64_t B, uint64_t seed, uint32_t call,
                             const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int chunks_requested);
/* Own minibatch per sample (upstream's use_own_batch_per_sample=True): the target above with a row list R_n of its own for every
 * sample n, n the sample's index IN THE CALL (never inside a tile, slab or launch).  For (seed, call), batch size B and T rows,
 * row j of sample n has the 64-bit stream position p = n B + j, epoch e = p div T and rank r = p mod T, and is data row
 *
 *     pi(r) = gmmvi_feistel_permute(r, e, call, stream 5, T, h, seed lo, seed hi)
 *
 * (csrc/feistel.h; the layout of the BNN stream, gmmvi_bnn_stream_origin_of / _row, on the data targets' stream id; NumPy:
 * minibatch_stream.data_minibatch_rows_per_sample).  R_n = { row j : 0 <= j < B } in the order of j, s = (float)T / (float)B.
 *   - sample 0's batch is exactly the shared batch of gmmvi_target_custom_data for the same (seed, call);
 *   - an epoch is one permutation of all rows, so within an epoch the batches of different samples are disjoint;
 *   - a batch that straddles an epoch boundary takes its tail from the next epoch's permutation and may hold one row twice;
 *   - B == T gives every sample its own permutation of all rows (sample n the whole of epoch n), with s = 1.
 * Range: N B may exceed 2^32 (p is formed in 64 bits); the epoch is at most (N B - 1) div T < N < 2^31 because B <= T,
 * which the entry checks like its sibling, so nothing wraps.
 * Kernels (csrc/custom_target_data.inc, gmmvi_data_rows_own_*): the geometry, the staged and direct x routes, the launch plan
 * (gmmvi_custom_data_plan with rows = B) and the order of the arithmetic of gmmvi_target_custom_data, unchanged: a wave adds its
 * positions j in order, wave 0 adds waves 1, 2, 3, chunks are added in index order, then s * sum, then + prior.  What differs:
 * the row is a per-lane value, so every lane walks the Feistel network for its own (sample, position) and reads its row through
 * vector loads; a gradient call repeats the walk in each of its ceil(D / W) passes (no index scratch).  The kernels and the bits
 * of gmmvi_target_custom_data are untouched.
 * Arguments of gmmvi_target_custom_data without the minibatch flag; the same refusals (B outside 1 .. T, T, C, N, D, the cap on D
 * for a gradient, NULL pointers, a handle of another mode or context), each before any launch, outputs untouched.  Profiling
 * tags: target_custom_data_own, target_custom_data_merge. */
int gmmvi_target_custom_data_own_batches(gmmvi_ctx* ctx, const gmmvi_custom_target* target, int D, const float* params_dev,
                                         const float* data_dev, int64_t T, int C, int64_t B, uint64_t seed, uint32_t call,
                                         const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int chunks_requested);

/* ---- differentiated user-defined targets on a tape: reverse mode ------------------------------------------------------------------
 * The forward mode above costs ceil(D / W) passes and stops at GMMVI_CUSTOM_AUTODIFF_MAX_DIM.  This mode takes the same source,
 *
 *     template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params);
 *
 * under the same rules, unchanged (a text that runs in the forward mode compiles and runs here; the compiler is additionally given
 * -DGMMVI_CUSTOM_TAPE=1, so a text can tell the modes apart), and gives the whole gradient from ONE recorded evaluation and one
 * backward sweep, at any D up to GMMVI_MAX_DIM_DIAG.  The library puts csrc/custom_target_tape.inc behind the source:
 *   - for a value call T = float, X = const float*, exactly as in the forward mode;
 *   - for a gradient call T = gmmvi_tape::Var, a value and a node id (id < 0: a constant; 0 <= id < D: the input x[id];
 *     id >= D: record id - D), and X is a view whose entry i is the input node i; reading it makes no record.
 * On a T the text defines the operations of the forward mode's list above, no more and no fewer, with the same partial
 * derivatives and tie rules (fabs at +-0, fmax / fmin ties, pow with exponent 0, the tanh form); a constant operand gets no
 * partial (the tape's form of "a direction in which the exponent does not move"), and an operation on constants alone makes no
 * record.  A T does not convert to float; gmmvi_value is the only way down.
 * One record is {int ia, ib; float pa, pb}: the parents' ids (ib = -1: one parent) and the partials, 16 bytes written by one
 * 16-byte store.  A wave's tape is laid out [record][64 lanes]: record r of a wave is 1 KiB of consecutive memory; the adjoints
 * have the same layout, 4 bytes per slot, and a record's adjoint is zeroed when the record is written.  Per lane and record that
 * is GMMVI_CUSTOM_TAPE_RECORD_BYTES of scratch.  The lane's record count is its own; all tape traffic is ordinary per-lane vector
 * loads and stores.
 * A call of gmmvi_dot, gmmvi_sqdist or gmmvi_sumsq on the input view makes one record of another kind, whatever n is (none for
 * n <= 0): ia = -2 - (4 n + kind), kind 0, 1, 2 in that order; ib = first; {pa, pb} hold the 64-bit address of c, or the bits of
 * center in pa.  ia == -1 still means a constant parent, and the records of every other operation keep their bits.  The sweep
 * that meets such a record with adjoint w adds c[i] w, 2 (x[first + i] - c[i]) w or 2 (x[first + i] - center) w to the adjoint of
 * input first + i for i < n, i ascending; it reads c and the lane's x then, after the user's function has returned.  A lane
 * sweeps the kind of its own record, whatever the other lanes of its wave hold at that record index.
 * Kind 3 is the node-array record of gmmvi_wdot and gmmvi_logsumexp, which spans 1 + ceil(n / 2) slots.  The payload comes
 * first: slot j = {id of entry 2 j, id of entry 2 j + 1 or -1, 32 bits for each entry}, the bits h[i].v for gmmvi_wdot and the
 * partial p_i for gmmvi_logsumexp.  The header stands behind its payload, because the sweep walks backwards:
 * {ia = -2 - (4 n + 3), ib = first or -1, the operation (0 gmmvi_wdot, 1 gmmvi_logsumexp), 0}.  The result's node id is the
 * header's; no node refers to a payload slot, and the adjoint zeroed for it is never read.  The loop forms cost 2 n and n - 1
 * records.  Beyond the capacity nothing is stored and the count advances slot by slot, so the needed length is in slots and the
 * relaunch is the usual one.  On a header with adjoint w, i ascending: gmmvi_wdot adds h[i].v w to the adjoint of input
 * first + i and, for an entry that is not a constant, x[first + i] w to the entry's adjoint (the gradient's entry if the entry
 * is an input); gmmvi_logsumexp adds p_i w to the adjoint of every entry that is not a constant.  Then the sweep steps over the
 * payload.
 * The overloads on tape nodes and this branch of the sweep are compiled only into a text that names gmmvi_wdot or gmmvi_logsumexp
 * (the library searches the source for the two names and defines GMMVI_TAPE_NODES): the kernels of every other source are what
 * they were without the two primitives.  A text that builds the name by token pasting therefore does not compile on the tape.
 * gmmvi_affine makes one record GROUP of ceil(n / 2) + 2 + m slots: the payload of gmmvi_wdot (the ids and the bits of h, once
 * for all m outputs; every entry of the const float* overload is a constant), two descriptor slots {w, si, sj, b} and
 * {sb, m, 0, 0}, then m headers {-2 - (4 n + 3), j, 2, 0}: the node-array kind with operation 2.  out[j] is the node of header
 * j; no Var refers to a payload or descriptor slot; beyond the capacity nothing is stored and the count advances slot by slot.
 * The sweep, walking backwards, meets some header j of the group first: header m - 1 where a later record consumed the outputs,
 * any j where the function's output is out[j] (records made after the output are never visited).  The adjoints a_0 .. a_j of
 * out[0 .. j] are final by then, and this one visit handles them all, in one fixed order: entry i ascending reads its payload
 * once and, jj ascending from 0 to j, adds h[i].v a_jj to the gradient of weight (i, jj) and gathers the sum over jj of
 * x[w + i si + jj sj] a_jj by fmaf from 0, which it adds once to the entry's adjoint (the gradient entry where the entry is an
 * input, nothing for a constant); then a_jj goes to the gradient of bias jj, jj ascending.  The sweep then steps back over
 * j + 1 + 2 + ceil(n / 2) slots: no other header of the group is visited.  No atomics: the same inputs give the same bits.
 * The overloads and this branch are compiled only into a text that names gmmvi_affine (GMMVI_TAPE_AFFINE, with which the library
 * defines GMMVI_TAPE_NODES too): the kernels of every other source, those that call gmmvi_wdot or gmmvi_logsumexp included, are
 * what they were.
 * Kernels: one lane is one sample, one wave per workgroup.  The lane records the user's function (every store guarded by the
 * capacity; beyond it the value stays right and the count keeps counting), then, in the same launch, seeds the output's adjoint
 * with 1 and walks its own records from the output back to the first.  Adjoints of inputs add up in the lane's own row of
 * grad_out_dev, which the lane zeroes first.  No atomic takes part in a floating-point sum: the same inputs give the same bits.
 * An output that is an input or a constant is handled; lanes past N write nothing.  Every lane raises the call's needed length
 * to its own count with an integer atomic maximum; a lane whose count exceeds the capacity writes no gradient.
 * Capacity: tape_capacity == 0 means what this handle has needed at this D so far (first use: GMMVI_CUSTOM_TAPE_DEFAULT_CAPACITY).
 * After a gradient launch the call reads the needed length back (4 bytes); if it exceeds the capacity, the scratch grows and the
 * launch is repeated once: values are deterministic, so the second run is the result.  The handle remembers the longest length
 * per D, so a steady-state call launches once.  THE READBACK IS A STREAM SYNCHRONISATION: this mode is a target of the modular
 * path only.  gmmvi_target_custom, and so target kind 5 of the single-call and the sharded iteration, refuse a tape handle.
 * Scratch: scratch_bytes == 0 means GMMVI_CUSTOM_TAPE_SCRATCH_BYTES, a setting, not a measurement.  If the lanes of N samples
 * (rounded up to whole waves) times capacity times GMMVI_CUSTOM_TAPE_RECORD_BYTES exceed the budget, the samples are processed
 * in slabs of a multiple of 64 lanes, launched one after another on the stream (gmmvi_custom_tape_plan).  A capacity that does
 * not fit the budget for 64 lanes is cut to what fits; if the launch then reports a longer tape, the call fails with
 * GMMVI_ERR_ARG, and the message states the needed length and its bytes (lp_out_dev is then written, grad_out_dev incomplete).
 * The scratch is the context's, reused across calls. */
#define GMMVI_CUSTOM_TAPE_RECORD_BYTES 20            /* 16 B of record + 4 B of adjoint */
#define GMMVI_CUSTOM_TAPE_DEFAULT_CAPACITY 1024      /* records per lane of a handle's first gradient launch at a D */
#define GMMVI_CUSTOM_TAPE_SCRATCH_BYTES 2147483648ull /* default budget of the tape scratch: 2 GiB */
/* gmmvi_custom_target_check / _compile for this mode (a source without gmmvi_user_density: GMMVI_ERR_ARG, the log names it).
 * The handle is an ordinary gmmvi_custom_target, released by gmmvi_custom_target_release; the mode is part of the context's
 * key: the same text compiled for the forward mode and for the tape gives two handles. */
int gmmvi_custom_target_check_tape(const char* source, const char* arch, char* log_out, size_t log_cap);
int gmmvi_custom_target_compile_tape(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out);
/* The slab plan, a host function (no device, no context): as many whole waves as scratch_bytes (0: the default) holds at
 * `capacity` records per lane form a slab, the slabs are as even as whole waves allow, *lanes_per_slab is a multiple of 64,
 * *slabs * *lanes_per_slab >= N and the last slab is never empty.  N < 1, capacity < 1, a NULL output, or a budget below the
 * need of 64 lanes: GMMVI_ERR_ARG. */
int gmmvi_custom_tape_plan(int N, int capacity, size_t scratch_bytes, int* slabs, int* lanes_per_slab);
/* *length = the longest tape (records per lane) a gradient launch of this handle has needed at D; 0: none yet. */
int gmmvi_custom_tape_length(gmmvi_ctx* ctx, const gmmvi_custom_target* target, int D, int* length);
/* lp[n] (and grad[n] when grad_out_dev != NULL) of the density.  X_dev[N,D], lp_out_dev[N], grad_out_dev[N,D] or NULL (one
 * launch of the float instantiation, no tape, no synchronisation).  GMMVI_ERR_ARG before any launch: N < 1; D outside
 * 1 .. GMMVI_MAX_DIM_DIAG; tape_capacity < 0; a NULL X_dev or lp_out_dev; a handle of another mode (the message names the entry
 * points) or context.  Profiling tag: target_custom_tape. */
int gmmvi_target_custom_tape(gmmvi_ctx* ctx, const gmmvi_custom_target* target, int D, const float* params_dev,
                             const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int tape_capacity,
                             size_t scratch_bytes);
/* One operation of the tape's number type on a host tape (no device, no context): op indexes the operations in the order of
 * gmmvi_autodiff_probe; a / b: the operands, each the input node 0 / 1 or, with its flag set, a constant (a float operand of the
 * operation is a float whatever its flag says).  *value: the result; *pa, *pb: the partials the operation recorded for a and b
 * (0 where it recorded none: a constant or float operand, a comparison, gmmvi_value); *records: the records it made.  An
 * unknown op or a NULL output: GMMVI_ERR_ARG. */
int gmmvi_tape_probe(int op, float a, float b, int a_is_const, int b_is_const, float* value, float* pa, float* pb, int* records);
/* The same for the special functions: op indexes the operations in the order of gmmvi_autodiff_probe_special. */
int gmmvi_tape_probe_special(int op, float a, float b, int a_is_const, int b_is_const, float* value, float* pa, float* pb,
                             int* records);
/* The same for the one-operand functions of gmmvi_autodiff_probe_extra, in its order. */
int gmmvi_tape_probe_extra(int op, float a, int a_is_const, float* value, float* pa, int* records);
/* One vector primitive on host arrays, op and the arrays as for gmmvi_autodiff_probe_vector: *value, *records (1, or 0 for
 * n <= 0), and grad[D], what the sweep of the tape modes leaves from that one node with adjoint 1 (0 outside
 * [first, first + n)).  An unknown op, a NULL array, D < 1, first < 0 or first + n > D: GMMVI_ERR_ARG. */
int gmmvi_tape_probe_vector(int op, const float* x, int D, int first, int n, const float* c, float center, float* value, float* grad,
                            int* records);
/* One primitive on an array of nodes, op and the array as for gmmvi_autodiff_probe_nodes (an entry that is not a constant is
 * one tanh record): *value; *records, the lane's count: the entries that are not constants plus the 1 + ceil(n / 2) slots of
 * the node-array record, the latter left out where the result is a constant; grad[D], what the sweep of the tape modes leaves
 * from the result with adjoint 1.  The same arguments are GMMVI_ERR_ARG. */
int gmmvi_tape_probe_nodes(int op, const float* x, int D, int first, int n, int src, int every, float* value, float* grad,
                           int* records);
/* The same call on an array whose entries are the input nodes themselves, h[i] = x[src + i] (they make no record, so *records
 * is 1 + ceil(n / 2) or 0), which may be -inf: the gradient of gmmvi_logsumexp is then its partials p_i bit for bit. */
int gmmvi_tape_probe_nodes_inputs(int op, const float* x, int D, int first, int n, int src, float* value, float* grad, int* records);
/* One gmmvi_affine call on a host tape: the arguments, the array and the output of gmmvi_autodiff_probe_affine (an entry that
 * is neither a constant, nor an input, nor a float is one tanh record).  values[m]: out[0 .. m); *records: the lane's count
 * behind the gmmvi_affine call, the entries' records plus ceil(n / 2) + 2 + m (0 more for n == 0 or m == 0), in front of the
 * gmmvi_logsumexp of pick == -1; *value and grad[D]: the output and what the sweep of the tape modes leaves from it with adjoint
 * 1, entering the group at header pick, or at header m - 1 from the record of the gmmvi_logsumexp.  The same arguments are
 * GMMVI_ERR_ARG. */
int gmmvi_tape_probe_affine(const float* x, int D, int w, int si, int sj, int b, int sb, int n, int m, int src, int every, int inputs,
                            int floats, int pick, float* values, float* value, float* grad, int* records);

/* ---- targets summed over a data set, differentiated on a tape ------------------------------------------------------------------
 * The source of the data mode, unchanged (gmmvi_user_row and gmmvi_user_prior, templates over the number type; compiled with
 * -DGMMVI_CUSTOM_TAPE=1), with the gradient from reverse mode at any D up to GMMVI_MAX_DIM_DIAG: forward mode makes ceil(D / 16)
 * passes over every row and stops at GMMVI_CUSTOM_AUTODIFF_MAX_DIM.  The library puts the whole text of the data mode, the
 * tape's number type (csrc/custom_target_tape.inc, same records, partials and tie rules) and csrc/custom_target_data_tape.inc
 * behind the source.  The key of the module cache is (source, mode): the same text compiled by gmmvi_custom_target_compile_data
 * gives another handle.
 * Value call (grad_out_dev == NULL): the value call of gmmvi_target_custom_data, kernel for kernel and bit for bit; no tape, no
 * synchronisation.
 * Gradient call: one wave of 64 lanes per (tile of 64 samples, chunk of the row list), lane = sample.  For each row of its chunk
 * in order the lane resets its record count, records the row term on a tape of `capacity` records that is reused for every
 * row, adds the value to its sum and walks the records back from the output node into its column of the wave's [D][64] gradient
 * accumulator in scratch.  The tape is as long as the longest single row term or the prior, not the data sum.  A second kernel,
 * one wave per tile, adds the chunks' partials, scales, adds the prior and sweeps the prior, recorded on the same tape, into the
 * scaled accumulator, then writes lp and grad.
 * Summation order, fixed (no atomic takes part in a floating-point sum; two identical calls give identical bits): per lane the
 * rows of a chunk in position order, the adjoints of one row from the output's record back to record 0; chunks in index order;
 * then s * sum; then + prior (value), and the prior's adjoints in sweep order (gradient).
 * Capacity, as for gmmvi_target_custom_tape: tape_capacity == 0 means what this handle has needed at this D so far (first use:
 * GMMVI_CUSTOM_TAPE_DEFAULT_CAPACITY); every lane raises an integer maximum of its record counts over all rows and the prior; the
 * call reads it back (it SYNCHRONISES the stream: modular path only), remembers it (gmmvi_custom_tape_length) and, if it exceeded
 * the capacity, runs once more at that length with the same seed and call, hence the same rows.  A second overflow is
 * GMMVI_ERR_ARG (the source is not a pure function).  A lane whose tape overflows still computes values and adds no adjoints.
 * Scratch: 64 * (capacity * GMMVI_CUSTOM_TAPE_RECORD_BYTES + 4 D) bytes per tile and chunk within scratch_bytes (0:
 * GMMVI_CUSTOM_TAPE_SCRATCH_BYTES); tiles that do not fit together run in slabs, one after another on the stream.  x is read
 * from X_dev directly.  gmmvi_target_custom, gmmvi_target_custom_data and gmmvi_target_custom_tape refuse a handle of this mode,
 * and this entry refuses the other four kinds, with GMMVI_ERR_ARG and a message naming the right entry. */
int gmmvi_custom_target_check_data_tape(const char* source, const char* arch, char* log_out, size_t log_cap);
int gmmvi_custom_target_compile_data_tape(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out);
/* The plan of a gradient call on N samples and a row list of `rows` at dimension D and `capacity` records per lane (needs no
 * device).  Chunks: the request, or (0) enough that tiles * chunks waves reach four per compute unit of an MI355X but no fewer
 * than 8 rows per chunk unless there is one chunk (set by the rule of gmmvi_custom_data_plan, not measured); at most one per row
 * and at most what the budget holds.  Then as many tiles per slab as the budget holds.  The last chunk and the last slab are
 * never empty; chunks * tiles_per_slab waves never exceed the budget.  GMMVI_ERR_ARG: N < 1, rows outside 1 .. 2^31 - 1, D
 * outside 1 .. GMMVI_MAX_DIM_DIAG, capacity < 1, chunks_requested < 0, a NULL output, or a budget that cannot hold one tile with
 * one chunk (the message gives both byte counts). */
int gmmvi_custom_data_tape_plan(int N, int64_t rows, int D, int capacity, int chunks_requested, size_t scratch_bytes, int* chunks,
                                int* rows_per_chunk, int* slabs, int* tiles_per_slab);
/* Arguments and refusals of gmmvi_target_custom_data, without its cap on D for a gradient, plus tape_capacity >= 0 and
 * scratch_bytes as above.  Profiling tags: target_custom_data_tape, target_custom_data_tape_finish (gradient call);
 * target_custom_data, target_custom_data_merge (value call). */
int gmmvi_target_custom_data_tape(gmmvi_ctx* ctx, const gmmvi_custom_target* target, int D, const float* params_dev,
                                  const float* data_dev, int64_t T, int C, int minibatch, int64_t B, uint64_t seed, uint32_t call,
                                  const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int chunks_requested,
                                  int tape_capacity, size_t scratch_bytes);
/* gmmvi_target_custom_data_tape with an own minibatch per sample: the row lists R_n of gmmvi_target_custom_data_own_batches, the
 * arguments of gmmvi_target_custom_data_tape without the minibatch flag, its refusals, capacity and scratch rules.  A value call
 * is the value call of gmmvi_target_custom_data_own_batches, kernel for kernel and bit for bit.  A gradient call launches
 * gmmvi_data_tape_rows_own (csrc/custom_target_data_tape.inc: gmmvi_data_tape_rows with the lane's own row pointer; a slabbed
 * launch forms the stream position from the sample's index in the call) and the unchanged finish kernel; the plan is
 * gmmvi_custom_data_tape_plan with rows = B.  The readback of the tape length and the second attempt at the needed capacity use
 * the same (seed, call), hence the same rows.  Profiling tags: target_custom_data_tape_own, target_custom_data_tape_finish
 * (gradient call); target_custom_data_own, target_custom_data_merge (value call). */
int gmmvi_target_custom_data_tape_own_batches(gmmvi_ctx* ctx, const gmmvi_custom_target* target, int D, const float* params_dev,
                                              const float* data_dev, int64_t T, int C, int64_t B, uint64_t seed, uint32_t call,
                                              const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                                              int chunks_requested, int tape_capacity, size_t scratch_bytes);
/* The two lane bodies of csrc/custom_target_data_tape.inc on the host (no device, no context), lane stride 1, behind the
 * logistic-regression row term and prior of csrc/custom_data_tape_sample.hip (row = [features (D) | label], params = [prior mean,
 * prior std]): all arrays are host arrays, the row list is that of gmmvi_target_custom_data for (minibatch, B, seed, call), the
 * chunk plan is given and must cover the row list with a non-empty last chunk.  Writes lp[N] and *needed, the longest record
 * count of a row term or the prior; grad[N, D] is written only if *needed <= capacity.  GMMVI_ERR_ARG for a bad argument. */
int gmmvi_data_tape_probe(int D, const float* params, const float* data, int64_t T, int C, int minibatch, int64_t B, uint64_t seed,
                          uint32_t call, const float* X, int N, int chunks, int rows_per_chunk, int capacity, float* lp,
                          float* grad, int* needed);

/* ---- predictive density of a data-set target -------------------------------------------------------------------------------------
 * What a fitted posterior of the shape above is judged by: for samples X[N, D] of the approximation and an evaluation set
 * rows[M, C] (held-out rows, or the training rows for WAIC), with  l[n, m] = gmmvi_user_row<float>(x_n, D, rows[m], C, params)
 * (the float instantiation of a value call; the prior takes no part), per row m
 *
 *     lpd[m]  = log sum_n exp(l[n, m]) - log N      the log posterior-predictive density, max-shifted
 *     mean[m] = (1 / N) sum_n l[n, m]
 *     var[m]  = M2 / (N - 1),  M2 = sum_n (l[n, m] - mean[m])^2;  0 for N = 1          (the unbiased variance: WAIC's penalty)
 *
 * Kernels (csrc/custom_target_data.inc, in the code object of every handle of gmmvi_custom_target_compile_data and
 * gmmvi_custom_target_compile_data_tape): the geometry of the value call, grid ceil(N / 64) x chunks, 4 waves on the same 64
 * samples, lane = sample, x staged in LDS up to GMMVI_CUSTOM_STAGED_MAX_DIM; a workgroup owns rows_per_chunk consecutive rows of
 * the evaluation set, its wave w the positions w, w + 4, ... of them, the row wave-uniform.
 * Reduction order, all fp32, no atomics: for its row the wave reduces over its 64 lanes with an xor butterfly (1, 2, 4, ..., 32):
 * the maximum; with shift = the maximum if finite, else 0, the sum of exp(l - shift); the sum of l, divided by the tile's count
 * (the tile mean); the sum of (l - tile mean)^2.  Lanes past N take no part: -inf to the maximum, 0 to the sums, and the count is
 * the number of valid lanes.  One tile: lane 0 finishes the row in place.  More: lane 0 writes (max, sumexp, mean, M2) to the
 * context's scratch, tiles * M * 4 floats, and a second kernel (thread = row) merges the tiles IN TILE-INDEX ORDER: the
 * log-sum-exp pairs by rescaling both to the shift of the larger maximum, and with  delta = mean_t - mean, n' = n + c_t:
 * mean += delta c_t / n',  M2 += M2_t + delta^2 n c_t / n'.  Then  lpd = (shift + log sumexp) - log N.
 * The same inputs give the same bits, and so does every chunk request: chunks split the rows, never a reduction.
 * Edge values of lpd: a column that is -inf at every sample gives -inf exactly (no -inf - (-inf): the shift is 0, and a partial
 * whose sumexp is 0 is not rescaled); -inf at some samples gives the finite log-sum of the others; a +inf gives +inf; a NaN gives
 * NaN (fmaxf drops it, the sum of exponentials carries it).  mean and var of a column that holds a non-finite value are whatever
 * IEEE arithmetic gives; only lpd has guaranteed handling.
 * The plan, a host function (no device, no context): *tiles = ceil(N / 64); *chunks and *rows_per_chunk by the rules of
 * gmmvi_custom_data_plan over the M evaluation rows: auto (0) enough chunks that tiles * chunks reaches 256 but at most M / 32,
 * at least 1; a request is honoured up to one row per chunk (and 65535); then rows_per_chunk = ceil(M / chunks), chunks =
 * ceil(M / rows_per_chunk), the last chunk never empty.  N < 1, M outside 1 .. 2^31 - 1, a negative request or a NULL output:
 * GMMVI_ERR_ARG. */
int gmmvi_custom_data_predictive_plan(int N, int64_t M, int chunks_requested, int* tiles, int* chunks, int64_t* rows_per_chunk);
/* lpd[M], and mean[M] / var[M] where the pointer is not NULL, of the handle's row term.  rows_dev[M, C] fp32, X_dev[N, D].
 * GMMVI_ERR_ARG before any launch, with a message: a NULL handle, rows_dev, X_dev or lpd_out_dev; a handle of another context; a
 * handle that was not compiled by gmmvi_custom_target_compile_data or gmmvi_custom_target_compile_data_tape (the message names
 * them); N < 1; M outside 1 .. 2^31 - 1; C < 1; D outside 1 .. GMMVI_MAX_DIM_DIAG; chunks_requested < 0.  No synchronisation.
 * Profiling tags: custom_data_predictive, custom_data_predictive_merge. */
int gmmvi_custom_data_predictive(gmmvi_ctx* ctx, const gmmvi_custom_target* target, int D, const float* params_dev,
                                 const float* rows_dev, int64_t M, int C, const float* X_dev, int N, float* lpd_out_dev,
                                 float* mean_out_dev, float* var_out_dev, int chunks_requested);
/* The tile reduction and the tile merge of those kernels on the host (no device, no context; csrc/predictive_probe.hip compiles
 * the very functions of the device text behind a 64-wide vector as the lane type) on a host matrix l[N, M] of row terms, for the
 * plan of (N, M, chunks_requested).  Writes lpd[M], mean[M], var[M]; a NULL array or a refused plan: GMMVI_ERR_ARG. */
int gmmvi_custom_data_predictive_probe(const float* l, int N, int64_t M, int chunks_requested, float* lpd, float* mean, float* var);

/* ---- sampling -------------------------------------------------------------------------------------------- */
/* x = mu_k + L_k eps for offsets[k] <= n < offsets[k+1] (component order), mapping[n] = k.
 * Replaces GMM.sample_from_components_no_shuffle + FullCovGMM.sample_from_component
 * (models/gmm.py:361-386, models/full_cov_gmm.py:36-39).  eps_dev[N,D] != NULL: host-provided normals
 * (bit-reproducible parity runs); else Philox4x32-10 keyed by seed, counter = first_index + n, given stream. */
int gmmvi_sample_components(gmmvi_ctx* ctx, int K, int D, const float* means_dev, const float* chols_dev,
                            const int32_t* offsets_dev, int N, uint64_t seed, uint64_t first_index, int stream_id,
                            const float* eps_dev, float* X_out_dev, int32_t* mapping_out_dev);
/* Standard normals eps[N,D] of the same Philox stream (tests, GMM.sample). */
int gmmvi_philox_normals(gmmvi_ctx* ctx, uint64_t seed, uint64_t first_index, int stream_id, int N, int D,
                         float* eps_out_dev);
/* Uniforms u[N] in (0,1): word 0 of block 0 (GMM.sample_categorical, models/gmm.py:134-137). */
int gmmvi_philox_uniforms(gmmvi_ctx* ctx, uint64_t seed, uint64_t first_index, int stream_id, int N,
                          float* u_out_dev);

/* ---- natural-gradient estimate (Stein) --------------------------------------------------------------------- */
/* SteinNgEstimator.get_expected_hessian_and_grad (gmmvi_modules/ng_estimator.py:204-263,171-188,154-169).
 * Inputs: packed model components, samples X[N,D], component log-densities ld[K,N] and model gradient
 * qgrad[N,D] (from gmmvi_mixture_eval on the same X), background densities bg[N], target gradients tgrad[N,D],
 * mapping[N] (only read with GMMVI_OWN_SAMPLES_ONLY; map_offset = K-1-max(mapping), ng_estimator.py:244).
 * Outputs: H_neg[K,D,D] = -E_k[...], g_neg[K,D]. */
int gmmvi_stein(gmmvi_ctx* ctx, int K, int D, const float* packed_dev, const float* X_dev, int N,
                const float* ld_dev, const float* qgrad_dev, const float* bg_dev, const float* tgrad_dev,
                const int32_t* mapping_dev, int map_offset, int flags, float* H_neg_out_dev, float* g_neg_out_dev);

/* MoreNgEstimator.get_expected_hessian_and_grad (gmmvi_modules/ng_estimator.py:296-376) with QuadFunc.fit_quadratic
 * (optimization/least_squares.py:126-191, RegressionFunc.fit :34-76): importance-weighted quadratic ridge regression of
 * the rewards tlp[n] - logq[n] on the samples whitened by each component; flags = enum gmmvi_stein_flags.
 * Inputs: packed blocks + chols[K,D,D] of the model, X[N,D], ld[K,N] and logq[N] (gmmvi_mixture_eval on the same X),
 * bg[N], tlp[N], mapping[N] (GMMVI_OWN_SAMPLES_ONLY only), l2[K] ridge coefficients (GmmWrapper.l2_regularizers).
 * Outputs: H_neg[K,D,D], g_neg[K,D]; NaN for a component whose ridge system is not positive definite.
 * D <= 63.  For a dimension on the blocked path (50 < D by default) the blocks handed over have another layout: the
 * components are re-packed in the register-path layout for the call (means from the blocks, factors from chols_dev);
 * D >= 64: GMMVI_ERR_ARG. */
int gmmvi_more(gmmvi_ctx* ctx, int K, int D, const float* packed_dev, const float* chols_dev, const float* X_dev, int N,
               const float* ld_dev, const float* logq_dev, const float* bg_dev, const float* tlp_dev,
               const int32_t* mapping_dev, int map_offset, int flags, const float* l2_dev, float* H_neg_out_dev,
               float* g_neg_out_dev);

/* The same estimate for 64 <= D <= GMMVI_MORE_BLOCKED_MAX_DIM (= 128): same arguments, flags and outputs as gmmvi_more, with
 * packed_dev in the blocked layout [mu | log-normaliser | pad | dense L^-1] (stride gmmvi_packed_stride(D)).  The samples
 * are whitened, and the estimate un-whitened, with the dense L^-1 of the blocks; chols_dev must be given and is not read.
 * The (F + 1)^2 fp64 Gram matrices (F = D(D+1)/2 + D + 1: 563 MB per component at D = 128) live in the context's
 * workspace; the components are processed in groups whose workspace stays under 8 GiB (environment GMMVI_MORE_WS_GB,
 * read per call, at least one component per group) with results that do not depend on the group size.
 * D outside 64 ... 128 (or D = 64 while GMMVI_BLOCKED_ABOVE = 64 keeps it on the register path) or a missing pointer:
 * GMMVI_ERR_ARG before any launch; a workspace the device cannot provide: GMMVI_ERR_HIP. */
int gmmvi_more_blocked(gmmvi_ctx* ctx, int K, int D, const float* packed_dev, const float* chols_dev, const float* X_dev,
                       int N, const float* ld_dev, const float* logq_dev, const float* bg_dev, const float* tlp_dev,
                       const int32_t* mapping_dev, int map_offset, int flags, const float* l2_dev, float* H_neg_out_dev,
                       float* g_neg_out_dev);

/* MORE for DIAGONAL-covariance mixtures (csrc/more_diag.hip; upstream has no diagonal branch, the definition is DESIGN.md
 * section 6): the regression of gmmvi_more on the sufficient statistics of a diagonal Gaussian, phi(z) = [z^2, z, 1] with
 * z = (x - mu) / sigma, F = 2 D + 1 features, bias unregularised, fp64 Gram matrix and Cholesky.  Needs function values of
 * the target only.  packed_dev: the diagonal component blocks of gmmvi_diag_pack (stride gmmvi_diag_packed_stride(D)); X, ld
 * (gmmvi_diag_mixture_eval on the same X), logq, bg, tlp, mapping, map_offset, flags and l2 as for gmmvi_more.
 * Outputs: h_neg_diag[K,D] (the diagonals, as gmmvi_diag_stein returns them) = -2 theta_quad / sigma^2 and
 * g_neg[K,D] = -theta_lin / sigma; NaN for a component whose ridge system is not positive definite.
 * 1 <= D <= GMMVI_MORE_DIAG_MAX_DIM (= 1024); the (F + 1)^2 fp64 Gram matrices (38 MB per component at D = 1024) live in the
 * context's workspace, components grouped under GMMVI_MORE_WS_GB as in gmmvi_more_blocked with results that do not depend on
 * the group size.  D outside 1 ... 1024 or a missing pointer: GMMVI_ERR_ARG before any launch. */
int gmmvi_more_diag(gmmvi_ctx* ctx, int K, int D, const float* packed_diag_dev, const float* X_dev, int N, const float* ld_dev,
                    const float* logq_dev, const float* bg_dev, const float* tlp_dev, const int32_t* mapping_dev,
                    int map_offset, int flags, const float* l2_dev, float* h_neg_diag_out_dev, float* g_neg_out_dev);

/* ---- component updates --------------------------------------------------------------------------------------- */
/* KLConstrainedNgBasedComponentUpdater.apply_NG_update (gmmvi_modules/ng_based_component_updater.py:431-524,
 * bracketing_search :335-429, kl :244-333) with the exact stop rules of SURVEY.md Appendix A.1.
 * In/out: means[K,D], chols[K,D,D], last_eta[K] (stores eta, not log eta; -1 = none), l2[K].
 * Out (may be NULL): success[K] (int32 0/1), kl[K], n_probes[K], packed[K, gmmvi_packed_stride(D)] = the Gaussian
 * parameter blocks of the updated model (saves the separate gmmvi_pack_components launch). */
int gmmvi_update_components_kl(gmmvi_ctx* ctx, int K, int D, float* means_dev, float* chols_dev,
                               const float* H_neg_dev, const float* g_neg_dev, const float* stepsizes_dev,
                               float temperature, float l2_init, float* last_eta_dev, float* l2_dev,
                               float* num_received_updates_dev, int32_t* success_out_dev, float* kl_out_dev,
                               int32_t* n_probes_out_dev, float* packed_out_dev);
/* Same contract, computed with the reference's own formulation (Q' = (eta Q + R)/eta, Cholesky + triangular inverse
 * per probe, sequential bisection).  Slow; kept as an on-device cross-check of the production kernel. */
int gmmvi_update_components_kl_reference(gmmvi_ctx* ctx, int K, int D, float* means_dev, float* chols_dev,
                                         const float* H_neg_dev, const float* g_neg_dev, const float* stepsizes_dev,
                                         float temperature, float l2_init, float* last_eta_dev, float* l2_dev,
                                         float* num_received_updates_dev, int32_t* success_out_dev, float* kl_out_dev,
                                         int32_t* n_probes_out_dev);
/* Test-only: the component-update step of the single-call iteration on its own -- the Stein moment partials of
 * (packed_old, X, ld, qgrad, bg, tgrad) followed by the update that finishes the estimate itself (directly from the moment sums,
 * in its finalize prologue, or after the stand-alone finalize launch).  H_neg[K,D,D] / g_neg[K,D] are scratch (written on the
 * explicit routes only); *slab_R_out (host, may be NULL) receives the number of partials per component. */
int gmmvi_stein_update_kl(gmmvi_ctx* ctx, int K, int D, const float* packed_old_dev, const float* X_dev, int N,
                          const float* ld_dev, const float* qgrad_dev, const float* bg_dev, const float* tgrad_dev,
                          int stein_flags, float* H_neg_dev, float* g_neg_dev, float* means_dev, float* chols_dev,
                          const float* stepsizes_dev, float temperature, float l2_init, float* last_eta_dev, float* l2_dev,
                          float* num_received_updates_dev, int32_t* success_out_dev, float* packed_out_dev,
                          int32_t* slab_R_out);
/* DirectNgBasedComponentUpdater (:97-141) and NgBasedComponentUpdaterIblr (:160-223). */
int gmmvi_update_components_direct(gmmvi_ctx* ctx, int K, int D, float* means_dev, float* chols_dev,
                                   const float* H_neg_dev, const float* g_neg_dev, const float* stepsizes_dev,
                                   float l2_init, float* l2_dev, float* num_received_updates_dev,
                                   int32_t* success_out_dev);
int gmmvi_update_components_iblr(gmmvi_ctx* ctx, int K, int D, float* means_dev, float* chols_dev,
                                 const float* H_neg_dev, const float* g_neg_dev, const float* stepsizes_dev,
                                 float l2_init, float* l2_dev, float* num_received_updates_dev,
                                 int32_t* success_out_dev);

/* ---- weights, rewards, stepsizes ---------------------------------------------------------------------------- */
/* WeightUpdater._get_expected_log_ratios (gmmvi_modules/weight_updater.py:56-75), self-normalised branch when
 * self_normalized != 0: E[k] = sum_n softmax_n(ld[k,n] - bg[n]) (tlp[n] - beta*logq[n]);
 * reward[k] = beta*logw[k] + E[k] (:73).  ess_out_dev (may be NULL) receives 1/sum_n w^2 per component
 * (sample_selector.py:154-158 uses the same weights). */
int gmmvi_expected_log_ratios(gmmvi_ctx* ctx, int K, int N, const float* ld_dev, const float* bg_dev,
                              const float* tlp_dev, const float* logq_dev, float beta, const float* logw_dev,
                              int self_normalized, float* E_out_dev, float* reward_out_dev, float* ess_out_dev);
/* The same launch reading the log values of a component-split sweep as its R >= 2 chunk partials logq_parts_dev [R][N]
 * (logq[n] = log sum_r exp(parts[r][n]), merged while read): the form the single-call iteration uses after a deferred merge. */
int gmmvi_expected_log_ratios_parts(gmmvi_ctx* ctx, int K, int N, const float* ld_dev, const float* bg_dev,
                                    const float* tlp_dev, const float* logq_parts_dev, int R, float beta,
                                    const float* logw_dev, int self_normalized, float* E_out_dev, float* reward_out_dev,
                                    float* ess_out_dev);
/* TrustRegionBasedWeightUpdater (weight_updater.py:164-279) followed by GMM.replace_weights (models/gmm.py:173-181).
 * stepsize_dev[1] is the KL bound.  kl_eta_out_dev[2] (may be NULL) = (kl, eta). No-op when K == 1 (:275). */
int gmmvi_update_weights_kl(gmmvi_ctx* ctx, int K, float* logw_dev, const float* E_dev, const float* stepsize_dev,
                            float beta, float* kl_eta_out_dev);
/* DirectWeightUpdater (weight_updater.py:123-141). */
int gmmvi_update_weights_direct(gmmvi_ctx* ctx, int K, float* logw_dev, const float* E_dev,
                                const float* stepsize_dev, float beta);
/* ImprovementBasedComponentStepsizeAdaptation.update_stepsize (component_stepsize_adaptation.py:165-188):
 * rewards_prev/rewards_last are reward_history[:, -2] / [:, -1]. */
int gmmvi_component_stepsize_improvement(gmmvi_ctx* ctx, int K, float* stepsizes_dev, const float* rewards_prev_dev,
                                         const float* rewards_last_dev, float min_stepsize, float max_stepsize,
                                         float inc_factor, float dec_factor);
/* ImprovementBasedWeightStepsizeAdaptation._update_stepsize (weight_stepsize_adaptation.py:141-156).
 * state_dev[2] = (stepsize, previous elbo proxy); updated in place. */
int gmmvi_weight_stepsize_improvement(gmmvi_ctx* ctx, int K, const float* logw_dev, const float* rewards_last_dev,
                                      float* state_dev, float min_stepsize, float max_stepsize, float inc_factor,
                                      float dec_factor);

/* ---- single-call iteration ------------------------------------------------------------------------------------- */
/* The built-in target of an iteration, described once for both plans below.  Only the members of `kind` are read. */
typedef struct gmmvi_target_spec {
    int32_t kind;                         /* 0: mixture family (gmmvi_mixture_eval), 1: planar robot, 2: logistic regression,
                                           * 4: Talos (gmmvi_target_talos), 5: user-defined (gmmvi_target_custom, route 0); any other
                                           * value, 3 included (no target has it): GMMVI_ERR_ARG */
    /* kind 0 */
    int32_t mix_family, mix_K;            /* enum gmmvi_family, number of target components */
    float mix_nu;
    const float* mix_packed;              /* [mix_K, stride] */
    const float* mix_logw;                /* [mix_K] */
    /* kind 1 (gmmvi_target_planar) */
    const float* planar_prior_std;        /* [D] */
    const float* planar_goals;            /* [planar_goals_count, 2] */
    int32_t planar_goals_count;
    float planar_likelihood_std;
    /* kind 2 (gmmvi_target_logreg): the signed data matrix [logreg_M, D], the isotropic normal prior */
    const float* logreg_A;
    int32_t logreg_M;
    float logreg_prior_mean, logreg_prior_std;
    /* kind 4 (gmmvi_target_talos, D == 34): the packed model table, the left gripper's goal [3] */
    const float* talos_model;
    const float* talos_context;
    /* kind 5 (gmmvi_target_custom): the compiled target (NULL: GMMVI_ERR_ARG) and its params_dev (may be NULL) */
    const gmmvi_custom_target* custom;
    const float* custom_params;
} gmmvi_target_spec;
/* One stepsize rule (component_stepsize_adaptation.py:165-188, weight_stepsize_adaptation.py:141-156). */
typedef struct gmmvi_stepsize_rule {
    int32_t mode;                         /* 0 fixed, 1 improvement-based (the bounds and factors are read for 1 only) */
    float min, max, inc, dec;
} gmmvi_stepsize_rule;
/* sizeof of the structs a binding has to mirror by hand: 0 gmmvi_target_spec, 1 gmmvi_stepsize_rule, 2 gmmvi_samtron_plan,
 * 3 gmmvi_sharded_plan; anything else: 0.  Needs no device. */
size_t gmmvi_struct_bytes(int which);

/* GMMVI.train_iter() (optimization/gmmvi.py:146-174) for the SAMTRON design choices with a component-based sample
 * selector: Stein estimator, KL-constrained component update, trust-region or direct weight update, improvement-based or
 * fixed stepsizes, built-in target.  The call is exactly the composition of the entry points above in the order the plug-in
 * modules invoke them (one host call instead of ~20), operating on the caller's state arrays.
 * Sample reuse (sample_selector.py:204-219, ratio_reused_samples_to_desired > 0): the caller has chosen the per-component
 * counts of the NEW samples (`offsets`; they follow from the effective sample sizes of the reused ones, sample_selector.py:
 * 160-202) and passes the number of reused samples `n_old`: the active samples are the n_old database rows in front of the
 * append position followed by the N new ones (contiguous in the database), the background mixture is given by
 * (bg_K, bg_packed, bg_logw) over the database's component snapshots of that window (sample_db.py:216-227).  With
 * n_old == 0 and bg_packed == NULL the background components are the model's own (one sweep for both). */
typedef struct gmmvi_samtron_plan {
    int32_t K, D, N;                      /* components, dimension, samples of this iteration (sum of the counts) */
    gmmvi_target_spec target;             /* checked before the rest of the plan */
    /* model state (in/out) */
    float* means; float* chols; float* logw;          /* [K,D], [K,D,D], [K] */
    const float* packed;                  /* parameter blocks of the CURRENT components [K, stride] */
    float* packed_new;                    /* out: blocks of the updated components */
    float* stepsizes; float* last_eta; float* l2; float* num_updates;      /* [K] each */
    int32_t* success_out;                 /* [K] or NULL */
    /* sampling */
    const int32_t* offsets;               /* [K+1] prefix sums of the per-component sample counts */
    int32_t max_per_component;            /* largest per-component count (0: N / K rounded up) */
    int32_t n_old;                        /* reused samples in front of the append position (0: none) */
    int32_t bg_K;                         /* n_old > 0: components the reused samples came from (snapshots; the new ones excluded) */
    const float* bg_packed;               /* [bg_K, stride] their snapshot blocks, or NULL (n_old == 0) */
    const float* bg_logw;                 /* n_old == 0: [K] log(count / N), the background weights (sample_db.py:225-226);
                                           * n_old > 0: [bg_K] log(count / n_old) of the components the reused samples came from */
    const float* bg_old;                  /* n_old > 0: [n_old] background density of the reused samples under those components with
                                           * those weights (what get_newest_samples(n_old) returned for the effective sample sizes) */
    const float* bg_logw_new;             /* n_old > 0: [K] log(count / N) of the new samples */
    float bg_log_share_old, bg_log_share_new;   /* n_old > 0: log(n_old / (n_old + N)), log(N / (n_old + N)) */
    uint64_t seed, first_index;           /* Philox key / global index of the first new sample */
    /* SampleDB append targets, already offset to the first free row (sample_db.py:115-124); snapshots may be NULL */
    float* db_samples; float* db_tlp; float* db_tgrad; int32_t* db_mapping; int32_t mapping_base;
    float* db_means; float* db_chols; float* db_packed;
    /* reward / weight history slots (models/gmm_wrapper.py:150-158,182) */
    const float* reward_prev; const float* reward_last; float* reward_next; float* weight_slot;
    float* wstate;                        /* [2]: weight stepsize, previous ELBO proxy */
    /* hyper-parameters */
    float temperature, l2_init;
    gmmvi_stepsize_rule component_stepsize, weight_stepsize;   /* applied to `stepsizes` / `wstate` ahead of the updates */
    int32_t weight_update_mode;           /* 0 trust-region, 1 direct */
    int32_t stein_flags;                  /* enum gmmvi_stein_flags (own-samples-only is not supported here;
                                           * GMMVI_EXPLICIT_ESTIMATE: results bit-equal to the module-by-module calls) */
    /* Drawing the NEXT iteration's samples early (n_old == 0 only).  x = mu + L eps needs the updated components, not the
     * weights (sample_selector.py:204-219), so the draw of iteration i + 1 can ride as extra workgroups in the post-update
     * sweep of iteration i instead of opening iteration i + 1 with a launch of its own.
     * presample_next != 0: after the component update, draw the N samples of the next iteration (same offsets, Philox
     *   indices first_index + N ..) into db_samples + N * D and their mapping (base mapping_base + K) into db_mapping + N;
     *   the caller has reserved those rows.
     * presampled != 0: db_samples / db_mapping already hold this iteration's draw (made by the previous call with
     *   presample_next, nothing touched the components, the offsets or the database since): no sampling launch. */
    int32_t presample_next, presampled;
    /* 0: the whole iteration.  1 / 2: the iteration in two calls -- 1 ends behind the component update, 2 is the weight
     * update (post-update sweep, expected log-ratios, weight step).  Between the two the caller may queue work that needs the
     * updated components but not the weights: with sample reuse the effective sample sizes of the NEXT iteration's window
     * (sample_selector.py:140-202), read back asynchronously, so that the next iteration starts without waiting for them. */
    int32_t phase;
} gmmvi_samtron_plan;
int gmmvi_train_iter_samtron(gmmvi_ctx* ctx, const gmmvi_samtron_plan* plan);

/* The same iteration for COMPONENT SHARDS (the reference has no multi-GPU code): rank r owns K components, their
 * samples and their updates; every component needs all N samples of the iteration, so the iteration has three exchange points.
 * It is issued as FOUR calls with one all-gather between consecutive calls (gmmvi_allgather_f32 in place on the exchange
 * buffers; the caller may substitute any exchange, e.g. through the host in tests) -- the launches inside a phase are those of
 * gmmvi_train_iter_samtron (packed density sweeps with carried merges, Stein slab whitened inside the update kernel):
 *   phase 1  draw the local samples and evaluate the target on them, straight into this rank's part of e1
 *   -- all-gather e1 --  [x | log p~ | grad log p~ | E | reward] of every rank
 *   phase 2  de-interleave e1; apply the PREVIOUS iteration's weight step from the gathered (E, reward) (replicated on every
 *            rank: nothing reads the new weights or the new reward column earlier); stepsize rules; dual density sweep over
 *            the local components on all N samples into this rank's part of e2
 *   -- all-gather e2 --  [background partial | log q partial | gradient partial] of every rank
 *   phase 3  combine the ranks' partials; Stein estimate and KL-constrained update of the local components; post-update
 *            sweep, its log q partial into this rank's part of e3
 *   -- all-gather e3 --
 *   phase 4  expected log-ratios and rewards of the local components into this rank's part of e1 (they travel with the next
 *            iteration's first exchange)
 * With n_ranks == 1 the gathers are no-ops and the gathered views may alias the parts. */
typedef struct gmmvi_sharded_plan {
    int32_t n_ranks, rank;
    int32_t K, D, N;                      /* LOCAL components, dimension, samples of ALL ranks (N % n_ranks == 0) */
    gmmvi_target_spec target;             /* as in gmmvi_samtron_plan */
    /* local model state (in/out) */
    float* means; float* chols; const float* packed; float* packed_new;
    float* stepsizes; float* last_eta; float* l2; float* num_updates; int32_t* success_out;
    float* logw_all;                      /* [K * n_ranks] replicated log weights */
    const float* bg_logw;                 /* [K] log(count_k / N) of the local components */
    const int32_t* offsets;               /* [K+1] prefix sums of the local per-component sample counts */
    int32_t max_per_component;
    uint64_t seed, first_index;           /* Philox key / global index of this rank's first new sample */
    /* exchange buffers [n_ranks * stride] floats; this rank's part at rank * stride */
    float* e1;                            /* stride (N / n_ranks) * (2 D + 1) + 2 K */
    float* e2;                            /* stride N * (D + 2) */
    float* e3;                            /* stride N */
    /* gathered arrays written by phase 2 */
    float* x_all; float* tlp_all; float* tgrad_all;      /* [N,D], [N], [N,D] */
    float* E_all; float* reward_all;      /* [K * n_ranks] */
    int32_t has_pending;                  /* e1 carries the previous iteration's (E, reward): phase 2 applies that weight step */
    float* reward_col_pending;            /* [K * n_ranks] reward-history column that receives the gathered rewards */
    const float* reward_prev; const float* reward_last;  /* [K] local slices of the two newest columns AFTER the pending step */
    const float* reward_last_all;         /* [K * n_ranks] the newest column (weight stepsize rule) */
    float* wstate;                        /* [2] weight stepsize, previous ELBO proxy */
    float temperature, l2_init;
    gmmvi_stepsize_rule component_stepsize, weight_stepsize;
    int32_t stein_flags;
    /* as in gmmvi_samtron_plan: phase 4 draws the NEXT iteration's local samples (Philox indices first_index + N ..) into this
     * rank's part of e1 as riders of the expected-log-ratio launch; phase 1 of a call with presampled != 0 skips its draw */
    int32_t presample_next, presampled;
    /* scratch that lives across the four phases (component log densities, merged mixture arrays): caller-owned so that
     * several plans can take turns on one context; at least gmmvi_sharded_scratch_floats(K, D, N) floats */
    float* scratch;
} gmmvi_sharded_plan;
size_t gmmvi_sharded_scratch_floats(int K, int D, int N);
int gmmvi_train_iter_sharded_phase(gmmvi_ctx* ctx, const gmmvi_sharded_plan* plan, int phase /* 1..4 */);

/* ---- multi-GPU exchange (component shards) ----------------------------------------------------- */
/* RCCL communicator over the ranks of one node; unique_id is the 128-byte ncclUniqueId produced by rank 0. */
int gmmvi_comm_unique_id(char* out_id_128);
int gmmvi_comm_init(gmmvi_ctx* ctx, const char* unique_id_128, int n_ranks, int rank);
int gmmvi_comm_destroy(gmmvi_ctx* ctx);
int gmmvi_allgather_f32(gmmvi_ctx* ctx, const float* send_dev, float* recv_dev, size_t count_per_rank);
int gmmvi_allreduce_f32(gmmvi_ctx* ctx, float* buf_dev, size_t count, int op /* 0 sum, 1 max */);
/* Combine per-rank partial mixtures: given gathered (lp_r[n], grad_r[n,D]) of R ranks, writes
 * lp[n] = LSE_r lp_r[n], grad[n] = sum_r exp(lp_r[n]-lp[n]) grad_r[n]  (the E2/E3 exchange of SURVEY.md 8e). */
int gmmvi_combine_partials(gmmvi_ctx* ctx, int R, int N, int D, const float* lp_parts_dev,
                           const float* grad_parts_dev, float* lp_out_dev, float* grad_out_dev);

/* ---- diagonal-covariance GMMs (models/diagonal_gmm.py:6-59) ---------------------------------------------------- */
/* chol[K,D] = sigma (square roots of the covariance diagonal).  Densities / gradients / sampling / background /
 * Stein CAN use the dense entry points above on L = diag(sigma) (kept for callers that hold dense factors; the Python mirror
 * uses the dedicated kernels below since round 3):
 * gmmvi_diag_embed writes dense[K,D,D] from diag[K,D]; gmmvi_diag_extract reads diag[K,D] = diagonal of dense[K,D,D]
 * (the diagonal Stein estimate of gmmvi_modules/ng_estimator.py:159-162,:178-181 is the diagonal of gmmvi_stein's
 * H_neg), both for D <= GMMVI_MAX_DIM_BLOCKED; gmmvi_reciprocal_f32 is SampleDB's inv_chols = 1 / chols
 * (optimization/sample_db.py:119,:130), any length. */
int gmmvi_diag_embed(gmmvi_ctx* ctx, int K, int D, const float* diag_dev, float* dense_out_dev);
int gmmvi_diag_extract(gmmvi_ctx* ctx, int K, int D, const float* dense_dev, float* diag_out_dev);
int gmmvi_reciprocal_f32(gmmvi_ctx* ctx, const float* src_dev, size_t n, float* dst_dev);
/* Dedicated O(D)-per-pair kernels for diagonal mixtures (csrc/diag_sweep.hip).  Component block of this path
 * (gmmvi_diag_pack, gmmvi_diag_packed_stride(D) floats): [mu | 1/sigma | 1/sigma^2 | log-normaliser | padding].
 *   gmmvi_diag_mixture_eval  DiagonalGMM.component_log_densities / log_density / log_density_and_grad (models/diagonal_gmm.py:
 *                            40-53, models/gmm.py:183-216,274-300) and SampleDB's background density over diagonal snapshots
 *                            (sample_db.py:164-228); logw2 / lp2_out: a second mixture over the same components (may be NULL)
 *   gmmvi_diag_sample        GMM.sample_from_components_no_shuffle for a DiagonalGMM (x = mu + sigma * eps,
 *                            models/diagonal_gmm.py:43-45): same offsets / Philox arguments as gmmvi_sample_components
 *   gmmvi_diag_stein         SteinNgEstimator, diagonal branches (ng_estimator.py:159-162,:178-181): h_neg_diag[K,D], g_neg[K,D];
 *                            arguments as gmmvi_stein
 * All four and gmmvi_diag_pack take 1 <= D <= GMMVI_MAX_DIM_DIAG.  Above GMMVI_MAX_DIM_BLOCKED the log-normaliser and the quadratic
 * form are accumulated in fp64 over the 32-dimension pieces (a log density is of size ~D there: its error stays near one fp32
 * ulp of the result at every D); up to GMMVI_MAX_DIM_BLOCKED the results are those of the fp32 sums, bit for bit. */
size_t gmmvi_diag_packed_stride(int D);
int gmmvi_diag_pack(gmmvi_ctx* ctx, int K, int D, const float* means_dev, const float* sigma_dev, float* packed_out_dev);
int gmmvi_diag_mixture_eval(gmmvi_ctx* ctx, int K, int D, const float* packed_dev, const float* logw_dev, const float* logw2_dev,
                            const float* X_dev, int N, float* ld_out_dev, float* lp_out_dev, float* grad_out_dev,
                            float* lp2_out_dev);
int gmmvi_diag_sample(gmmvi_ctx* ctx, int K, int D, const float* means_dev, const float* sigma_dev, const int32_t* offsets_dev,
                      int N, uint64_t seed, uint64_t first_index, int stream_id, const float* eps_dev, float* X_out_dev,
                      int32_t* mapping_out_dev);
int gmmvi_diag_stein(gmmvi_ctx* ctx, int K, int D, const float* packed_dev, const float* X_dev, int N, const float* ld_dev,
                     const float* qgrad_dev, const float* bg_dev, const float* tgrad_dev, const int32_t* mapping_dev,
                     int map_offset, int flags, float* h_neg_diag_out_dev, float* g_neg_out_dev);

/* KLConstrainedNgBasedComponentUpdater.apply_NG_update, diagonal branches (gmmvi_modules/
 * ng_based_component_updater.py:447-453, kl() :304-318, :483-490); same contract as gmmvi_update_components_kl with
 * chols[K,D] and H_neg[K,D].  1 <= D <= GMMVI_MAX_DIM_DIAG: up to GMMVI_MAX_DIM_BLOCKED one wavefront per component with the
 * component in registers; above, one workgroup per component with the per-dimension state in LDS (D <= 8192) or re-read from
 * global memory, the KL summed as the per-dimension terms log r + 1/r - 1 (r = new precision / precision).  Same stop
 * rules and outputs on both routes. */
int gmmvi_update_components_diag_kl(gmmvi_ctx* ctx, int K, int D, float* means_dev, float* chols_diag_dev,
                                    const float* H_neg_diag_dev, const float* g_neg_dev, const float* stepsizes_dev,
                                    float temperature, float l2_init, float* last_eta_dev, float* l2_dev,
                                    float* num_received_updates_dev, int32_t* success_out_dev, float* kl_out_dev,
                                    int32_t* n_probes_out_dev);
/* NgBasedComponentUpdaterIblr, diagonal branches (:170-174, :188-189, :195-197).  (The reference's direct updater
 * has no diagonal branch.)  1 <= D <= GMMVI_MAX_DIM_DIAG, routes as gmmvi_update_components_diag_kl. */
int gmmvi_update_components_diag_iblr(gmmvi_ctx* ctx, int K, int D, float* means_dev, float* chols_diag_dev,
                                      const float* H_neg_diag_dev, const float* g_neg_dev, const float* stepsizes_dev,
                                      float l2_init, float* l2_dev, float* num_received_updates_dev,
                                      int32_t* success_out_dev);

/* ---- MMD (experiments/evaluation/mmd.py:41-58) ------------------------------------------------------------------ */
/* sum_out = sum_{i<Na} sum_{j<Nb} exp(-sum_d inv_bandwidth[d] (A[i,d] - B[j,d])^2)  (fp32 pairs, fp64 sums, fixed
 * summation order).  compute_ustat(sample) is (A, B) = (sample, sample); kernel_mix(sample) is (groundtruth, sample);
 * inv_bandwidth[d] = 1 / (alpha * sigma[d,d]).  scratch_dev holds gmmvi_mmd_scratch_doubles(Na, Nb) doubles. */
size_t gmmvi_mmd_scratch_doubles(int Na, int Nb);
int gmmvi_mmd_pair_sum(gmmvi_ctx* ctx, const float* A_dev, int Na, const float* B_dev, int Nb, int D,
                       const float* inv_bandwidth_dev, double* scratch_dev, double* sum_out_dev);

#ifdef __cplusplus
}
#endif
#endif /* GMMVI_HIP_H */
