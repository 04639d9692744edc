/*
 * sehip.h -- C ABI of libsehip.so: the MI355X (gfx950) implementation of the cosine-embedding
 * training + retrieval hot path of cvjena/semantic-embeddings.
 *
 * The reference is pure Python (Keras/TF + NumPy) and has no FFI; every entry point below names
 * the reference Python interface it replaces (paths relative to the reference checkout) so a
 * maintainer can bind it with ctypes -- INTEGRATION.md shows the stubs.
 *
 * Conventions (all entry points):
 *   - plain C types only; every pointer is a DEVICE pointer unless marked "host";
 *   - row-major, innermost dimension contiguous, explicit leading dimensions in ELEMENTS;
 *   - the caller owns every buffer; scratch memory is sized by the *_workspace_bytes() queries
 *     and passed in -- the library never allocates device memory;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it.  Exceptions, each marked at its
 *     declaration: se_rank_rows_init and se_rank_rows_check synchronise the stream (they hand a verdict to the host), and
 *     se_rank_rows synchronises ONCE per process and device when se_rank_rows_init was not called first (see there);
 *   - return value: SE_OK (0) or a negative SE_ERR_* code; se_last_error() (thread-local text)
 *     explains the last failure; no exceptions; re-entrant, safe from any host thread.  Process-wide state is limited to
 *     read-mostly caches filled at first use: device properties (CU count, kernel occupancies), the plan table of
 *     se_retrieve_topk, and -- the only one that influences which kernel runs -- the per-device verdict of the ranking's
 *     capability probe / self-test (atomics; see se_rank_rows_init).  Three environment variables are read by the product build,
 *     all of them by the ranking only: SE_RANK_SAFE=1 (never use the hardware-ordered kernels), SE_RANK_CHECK=1 (audit every row
 *     of every se_rank_rows call: synchronises every call), SE_RANK_VERBOSE=1 (probe / self-test verdicts on stderr).  Results
 *     never depend on them; no other switch exists in libsehip.so (libsehip_tuning.so is the build with tuning switches);
 *   - float32 arithmetic on the bit-exact paths follows the "canonical arithmetic" of
 *     DESIGN.md section 3 (sequential fp32 FMA chain over k, NumPy pairwise row sums,
 *     ascending (distance, index) order, NaN last, -0 == +0).
 */
#ifndef SEHIP_H
#define SEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE_OK 0
#define SE_ERR_INVALID (-1)     /* bad argument (shape, null pointer, unsupported k ...) */
#define SE_ERR_HIP (-2)         /* a HIP runtime call / kernel launch failed              */
#define SE_ERR_UNSUPPORTED (-3) /* valid request that this build does not implement        */
#define SE_ERR_WORKSPACE (-4)   /* workspace too small                                     */

/* element type of the feature tensor handed to the loss kernels */
#define SE_DTYPE_F32 0
#define SE_DTYPE_BF16 1

/* distance / similarity flavours of the all-pairs kernel */
#define SE_METRIC_COSINE 0 /* out = -(a . b)              evaluate_retrieval.py:59  */
#define SE_METRIC_EUCLID 1 /* out = (|a|^2 + |b|^2) - 2ab evaluate_retrieval.py:61-62 */
#define SE_METRIC_DOT 2    /* out = a . b                 utils.py:90 (K.dot(y_pred, centroids)) */

typedef void *se_stream_t; /* hipStream_t */

int se_version(void);
const char *se_last_error(void);
/* host: name of the GPU architecture the embedded code objects were built for ("gfx950") */
const char *se_build_arch(void);

/*
 * Phase timing -- a measuring aid (bench.py's per-leg rooflines), not part of any result.  se_phase_timing(1): from now on the
 * multi-kernel entry points (se_retrieve_topk) record a HIP event on their stream behind each of their phases ("convert", "sample",
 * "threshold", "filter", "refine", "fallback") and count, per query, the candidates of the filter pass and the entries the
 * refinement recomputed exactly; se_phase_timing(0) (the default state) switches it off.  One process-wide switch; calls made while
 * it is on must not run concurrently.
 * se_phase_timing_read: waits for the last recorded event and returns the number of phases written to names_host / ms_host (HOST
 * arrays of `cap` entries, either may be NULL; a phase that ran several times appears several times, in order); counters_host (HOST,
 * 5 int64 or NULL) receives the statistics words of the last se_retrieve_topk call -- [1] queries redone exactly, [2] entries
 * recomputed with the exact chain, [3] candidates listed, [4] queries -- or -1 each; the workspace of that call must still be alive.
 * The recording restarts empty afterwards.  Negative return value: an SE_ERR_* code.
 */
int se_phase_timing(int on);
int se_phase_timing_read(const char **names_host, float *ms_host, int cap, int64_t *counters_host);

/* ------------------------------------------------------------------------------------------
 * Training side
 * ------------------------------------------------------------------------------------------ */

/*
 * Fused  l2norm  +  embedding gather  +  cosine loss  (forward).
 * Replaces: utils.l2norm (utils.py:125-127) wrapped as the model's last layer
 *           (learn_image_embeddings.py:127-128), transform_inputs' host gather embedding[y]
 *           (learn_image_embeddings.py:48-50), utils.inv_correlation (utils.py:44-46) and the
 *           Keras batch mean.
 *   x        [B, D] features (f32 or bf16, ldx elements between rows)
 *   labels   [B] int64 class indices in [0, C)
 *   emb      [C, D] f32 class embeddings (lde)
 *   xhat     [B, D] f32 out: x * rsqrt(max(sum x^2, 1e-12))        (may be NULL)
 *   inv_norm [B] f32 out: rsqrt(max(sum x^2, 1e-12))               (may be NULL)
 *   loss_i   [B] f32 out: 1 - sum_d emb[labels[i], d] * xhat[i, d]
 *   loss_mean[1] f32 out: mean_i loss_i, fixed summation order     (may be NULL)
 */
int se_cosine_loss_fwd(const void *x, int x_dtype, int64_t ldx, const int64_t *labels,
                       const float *emb, int64_t lde, int64_t B, int64_t D, int64_t C,
                       float *xhat, int64_t ldxhat, float *inv_norm, float *loss_i,
                       float *loss_mean, se_stream_t stream);

/*
 * Backward of the above (what TF autodiff derives from utils.py:44-46,125-127):
 *   g_i = -grad_loss_i[i] * emb[labels[i]]
 *   dx_i = (g_i - xhat_i (xhat_i . g_i)) * inv_norm_i      where sum x^2 >= 1e-12
 *   dx_i = g_i * inv_norm_i                                 where the max() clamp is active
 *   x [B,D] is re-read (f32/bf16); dx is written in dx_dtype (f32/bf16).
 *   grad_loss_i [B] f32 (upstream gradient per sample; 1/B for the plain batch mean);
 *   if grad_loss_i is NULL, grad_scale is used for every row.
 */
int se_cosine_loss_bwd(const void *x, int x_dtype, int64_t ldx, const int64_t *labels,
                       const float *emb, int64_t lde, const float *grad_loss_i, float grad_scale,
                       int64_t B, int64_t D, int64_t C, void *dx, int dx_dtype, int64_t lddx,
                       se_stream_t stream);

/*
 * Squared-distance loss of `--loss mse` against the gathered class embedding, and its backward.
 * Replaces: utils.squared_distance (utils.py:34-36) as the training loss (learn_image_embeddings.py:160-163) on
 *           y_true = embedding[y] (transform_inputs, learn_image_embeddings.py:48-50), and the utils.mean_distance metric
 *           (utils.py:39-41) of the same compile() call.
 *   loss_i [B] f32 = sum_d (x_d - emb[y]_d)^2;  dist_i [B] f32 = sqrt(loss_i) (may be NULL);  loss_mean [1] (may be NULL).
 *   bwd: dx [B, D] (f32 / bf16) = 2 w (x - emb[y]), w = grad_loss_i[row] (NULL: the scalar grad_scale, e.g. 1 / B).
 */
int se_sqdist_loss_fwd(const void *x, int x_dtype, int64_t ldx, const int64_t *labels, const float *emb,
                       int64_t lde, int64_t B, int64_t D, int64_t C, float *loss_i, float *dist_i,
                       float *loss_mean, se_stream_t stream);
int se_sqdist_loss_bwd(const void *x, int x_dtype, int64_t ldx, const int64_t *labels, const float *emb,
                       int64_t lde, const float *grad_loss_i, float grad_scale, int64_t B, int64_t D,
                       int64_t C, void *dx, int dx_dtype, int64_t lddx, se_stream_t stream);

/*
 * Stand-alone L2-normalisation head and its backward.
 * Replaces: utils.l2norm (utils.py:125-127) used as `Lambda(utils.l2norm, name='l2norm')`
 *           (learn_image_embeddings.py:127-128) when the normalised embedding itself is wanted
 *           (feature dumps, learn_image_embeddings.py:270-275; inference).
 *   xhat [B, D] f32 = x * rsqrt(max(sum x^2, 1e-12)); inv_norm [B] f32 and sumsq [B] f32 = sum x^2
 *   (each may be NULL in fwd).
 *   bwd: dx = (grad - xhat (xhat . grad)) * inv_norm where sumsq >= 1e-12, grad * inv_norm on the epsilon
 *   clamp; inv_norm and sumsq are the forward's.  (inv_norm alone cannot tell: sum x^2 = 1e-12f and the
 *   next float above it both give inv_norm = 1e6f.)
 */
int se_l2norm_fwd(const void *x, int x_dtype, int64_t ldx, int64_t B, int64_t D, float *xhat,
                  int64_t ldxhat, float *inv_norm, float *sumsq, se_stream_t stream);
int se_l2norm_bwd(const float *grad, int64_t ldg, const float *xhat, int64_t ldxhat,
                  const float *inv_norm, const float *sumsq, int64_t B, int64_t D, float *dx,
                  int64_t lddx, se_stream_t stream);

/*
 * Nearest-class-embedding accuracy metric.
 * Replaces: utils.nn_accuracy(embedding, dot_prod_sim, k) (utils.py:57-100): the dense
 *           contraction y_pred @ embedding.T (utils.py:90 / :78) on MFMA plus the
 *           |best - true| < 1e-6 test (top-k: any of the k best within 1e-6).
 *   y_pred  [B, D] f32 (already normalised when dot_prod_sim, as in the reference)
 *   labels  [B] int64; y_true of the reference is emb[labels]
 *   dot_prod_sim != 0: similarity = y_pred . emb^T, larger is better   (utils.py:87-95)
 *   dot_prod_sim == 0: squared Euclidean distance, smaller is better    (utils.py:73-85)
 *   acc     [B] f32 out (0/1)
 *   scores  [B, C] f32 out, the similarity / distance matrix           (may be NULL)
 *   best    [B] int32 out, argmax / argmin class (lowest index on ties) (may be NULL)
 *   workspace: se_nn_accuracy_workspace_bytes(B, C) bytes, 8-byte aligned (0 for small class sets: one workgroup then walks
 *           all class tiles of its 32 samples; large sets -- C = 1000 -- are cut into class slices whose partial counts meet there)
 */
int64_t se_nn_accuracy_workspace_bytes(int64_t B, int64_t C);
int se_nn_accuracy(const float *y_pred, int64_t ldp, const int64_t *labels, const float *emb,
                   int64_t lde, int64_t B, int64_t D, int64_t C, int dot_prod_sim, int k,
                   float *acc, float *scores, int64_t lds, int32_t *best, void *workspace,
                   int64_t workspace_bytes, se_stream_t stream);

/*
 * Embedding heads: the loss of `--loss inv_corr` / `--loss mse` AND the nearest-class metric of its batch in one forward launch.
 * Replaces: utils.inv_correlation on the l2norm head (utils.py:44-46, 125-127) or utils.squared_distance (utils.py:34-36), plus
 *           utils.nn_accuracy(embedding, dot_prod_sim, k) for every k (utils.py:57-100), which differ only in the last comparison.
 * The contract is bit identity with the entry points above, on the same inputs:
 *   mode 0 (cosine head): xhat, inv_norm, loss_i, loss_mean are the bits of se_cosine_loss_fwd (float32 or bf16 x, 1e-12 clamp,
 *           clamped labels); n_better, n_within, best, scores are what se_nn_accuracy(dot_prod_sim = 1) computes from that xhat.
 *   mode 1 (squared-distance head): loss_i, dist_i, loss_mean are the bits of se_sqdist_loss_fwd; the metric outputs are those of
 *           se_nn_accuracy(dot_prod_sim = 0) on x widened to float32.
 *   n_within [B] int32: classes whose score is within 1e-6 of the label's; n_better [B] int32: classes beyond it by >= 1e-6.
 *           The accuracy for any k is (n_within >= 1) && (n_better < k): the 0/1 value se_nn_accuracy(..., k, ...) writes.
 *   xhat, inv_norm (mode 0), dist_i (mode 1), loss_mean, best, scores may be NULL; the outputs of the other mode are ignored.
 *   The normalised features do not travel through memory between loss and metric: xhat is written only when it is asked for.
 *   workspace: se_embed_head_workspace_bytes(mode, B, D, C) bytes, 8-byte aligned (0 while one workgroup walks all class tiles of
 *           its 32 samples); the call zeroes what it needs of it on `stream`, so it can be captured in a HIP graph.
 *   B == 0 returns SE_OK and touches nothing; a bad mode, dtype, leading dimension, a null required pointer or a missing, short
 *   or misaligned workspace returns SE_ERR_INVALID.  Results do not depend on the launch geometry or on concurrent work.
 */
int64_t se_embed_head_workspace_bytes(int mode, int64_t B, int64_t D, int64_t C);
int se_embed_head_fwd(int mode, const void *x, int x_dtype, int64_t ldx, const int64_t *labels,
                      const float *emb, int64_t lde, int64_t B, int64_t D, int64_t C,
                      float *xhat, int64_t ldxhat, float *inv_norm, float *loss_i, float *dist_i,
                      float *loss_mean, int32_t *n_better, int32_t *n_within, int32_t *best,
                      float *scores, int64_t lds, void *workspace, int64_t workspace_bytes,
                      se_stream_t stream);

/*
 * Joint head of `--cls_weight`: the embedding loss on the model's first output, the cross-entropy of the classifier branch and the
 * metrics of both outputs in ONE forward launch; both gradients in one backward launch.
 * Replaces: utils.inv_correlation(embedding[y], p) (utils.py:44-46) as the loss of `--loss inv_corr | unnorm_corr | softmax_corr`
 *           beside a classifier branch (learn_image_embeddings.py:160-180), utils.nn_accuracy(embedding, True, k) for every k
 *           (utils.py:57-100) or, for one-hot-like targets, 'accuracy' and utils.top_k_acc (utils.py:49-54) on that output, Keras 2.2's
 *           'categorical_crossentropy' with 'accuracy' / utils.top_k_acc on the `prob` output, and what TF autodiff derives from both.
 *   p [B, D] f32 (ldp): the first output as it stands in the graph -- the l2norm layer's output for inv_corr, the softmax output for
 *           softmax_corr, the raw embedding for unnorm_corr.  It is NOT normalised again (the classifier branch reads the same tensor,
 *           which is why se_embed_head_fwd mode 0 cannot serve here).
 *   labels [B] int64, clamped to [0, C - 1].  C: the rows of emb AND the columns of logits.
 *   emb [C, D] f32 (lde), or NULL: the identity table of `--embedding onehot`, which needs D == C and SE_HEAD_METRIC_ARGMAX.
 * Embedding role:
 *   emb_loss_i [B] = 1 - dot(emb[y_i], p_i); the dot is the row chain of se_cosine_loss_fwd (its x . emb[y]), with that entry
 *           point's rule for the 16-byte path, so the summation order is fixed.  emb == NULL: the single operation 1.0f - p[i, y_i].
 *   SE_HEAD_METRIC_NEAREST: n_better, n_within [B] int32, p_best [B] int32 and scores [B, C] f32 (lds) are what
 *           se_nn_accuracy(dot_prod_sim = 1) computes from p, bit for bit; (n_within >= 1) && (n_better < k) is its 0/1 value for
 *           every k (see se_embed_head_fwd).  p_above is not written.
 *   SE_HEAD_METRIC_ARGMAX (needs D == C): one scan of the row of p itself.  p_best [B] int32 = its arg-max class with np.argmax's
 *           rules (lowest index on ties, the first NaN wins); p_above [B] int32 = the number of entries strictly greater than
 *           p[i, y_i].  p_best == y is Keras' accuracy, p_above < k is tf.nn.in_top_k.  Non-finite rows follow se_softmax_xent_fwd's
 *           best / above: a row with a NaN or +inf, or of nothing but -inf, has p_above = C.  n_better, n_within and scores are
 *           not written.
 * Classifier role (logits != NULL; [B, C] f32 / bf16, ldz): cls_loss_i [B], aux (se_softmax_xent_aux_floats(B) floats), z_best and
 *   z_above [B] int32 carry the bits of se_softmax_xent_fwd(smoothing = 0) on the same inputs -- it is the same row code.
 *   logits == NULL runs the embedding role alone (unnorm_corr / softmax_corr without --cls_weight).
 * Both roles run in one grid up to C = 8192 (the register paths of the cross-entropy); longer rows of logits take a second launch.
 * The bits do not depend on that, on the launch geometry or on concurrent work.
 *   bwd: dp [B, D] f32 (lddp): dp[i, d] = fl(-w_i * emb[y_i, d]); emb == NULL: -w_i at column y_i, +0 elsewhere.
 *        w_i = grad_emb_loss_i[i] (NULL: grad_emb_scale for every row).  dz [B, C] f32 / bf16 (lddz) carries the bits of
 *        se_softmax_xent_bwd(smoothing = 0) with grad_cls_loss_i / grad_cls_scale and the forward's aux.  Every element of dp and dz
 *        is written.  logits == NULL skips dz; dp == NULL skips the embedding role.
 *   workspace: se_joint_head_workspace_bytes(metric, B, D, C) bytes, 8-byte aligned (0 for the arg-max metric and while one
 *        workgroup walks all class tiles of its 32 samples); the call zeroes what it needs of it on `stream`.
 *   Asynchronous on `stream`, no allocation, no host synchronisation, integer atomics only: capturable in a HIP graph.
 *   B == 0 returns SE_OK and touches nothing.  SE_ERR_INVALID: a bad metric or dtype; a leading dimension below the width;
 *   emb == NULL with SE_HEAD_METRIC_NEAREST or D != C; SE_HEAD_METRIC_ARGMAX with D != C; a null required pointer (p, labels,
 *   emb_loss_i; n_better and n_within under SE_HEAD_METRIC_NEAREST; p_above under SE_HEAD_METRIC_ARGMAX; cls_loss_i and aux -- bwd:
 *   aux and dz -- whenever logits is given); a missing, short or misaligned workspace.  p_best, scores, z_best, z_above may be NULL.
 */
#define SE_HEAD_METRIC_NEAREST 0   /* nearest class embedding by dot product: n_better / n_within (utils.nn_accuracy, dot_prod_sim) */
#define SE_HEAD_METRIC_ARGMAX  1   /* arg-max of p itself against the label: p_best / p_above ('accuracy', utils.top_k_acc)      */
int64_t se_joint_head_workspace_bytes(int metric, int64_t B, int64_t D, int64_t C);
int se_joint_head_fwd(const float *p, int64_t ldp, const int64_t *labels, const float *emb, int64_t lde,
                      int64_t B, int64_t D, int64_t C, int metric,
                      float *emb_loss_i, int32_t *n_better, int32_t *n_within, int32_t *p_best, int32_t *p_above,
                      float *scores, int64_t lds,
                      const void *logits, int z_dtype, int64_t ldz, float *cls_loss_i, float *aux,
                      int32_t *z_best, int32_t *z_above,
                      void *workspace, int64_t workspace_bytes, se_stream_t stream);
int se_joint_head_bwd(const int64_t *labels, const float *emb, int64_t lde, int64_t B, int64_t D, int64_t C,
                      const float *grad_emb_loss_i, float grad_emb_scale, float *dp, int64_t lddp,
                      const void *logits, int z_dtype, int64_t ldz, const float *aux,
                      const float *grad_cls_loss_i, float grad_cls_scale, void *dz, int dz_dtype, int64_t lddz,
                      se_stream_t stream);

/*
 * Label-embedding baseline loss (Sun et al.), forward and backward.
 * Replaces: labelembed_loss(out1, out2, tar, targets, tau, alpha, beta) and cross_entropy
 *           (learn_labelembedding.py:17-37); the backward is what TF autodiff derives from it
 *           (softmax(out2 / tau), softmax(tar) inside L_o1_emb and the arg-max mask are stop_gradient).
 *   out1, out2, tar [B, C] f32 logits (ld* elements between rows); targets [B] int64
 *   loss_i [B] f32 out (the reference returns it as [B, 1], learn_labelembedding.py:54)
 *   aux    se_labelembed_aux_floats(B) floats, caller-owned: per-sample log-sum-exps, the mask and the
 *          batch scale B / (sum mask + 1e-8); written by fwd, read by bwd
 *   bwd: grad_loss_i [B] f32 upstream gradient (NULL: grad_scale for every sample);
 *        d_out1, d_out2, d_tar [B, C] f32 out, any of them may be NULL
 */
int64_t se_labelembed_aux_floats(int64_t B);
int se_labelembed_loss_fwd(const float *out1, int64_t ld1, const float *out2, int64_t ld2,
                           const float *tar, int64_t ldt, const int64_t *targets, int64_t B, int64_t C,
                           float tau, float alpha, float beta, float *loss_i, float *aux,
                           se_stream_t stream);
int se_labelembed_loss_bwd(const float *out1, int64_t ld1, const float *out2, int64_t ld2,
                           const float *tar, int64_t ldt, const int64_t *targets,
                           const float *grad_loss_i, float grad_scale, int64_t B, int64_t C, float tau,
                           float alpha, float beta, const float *aux, float *d_out1, int64_t ldd1,
                           float *d_out2, int64_t ldd2, float *d_tar, int64_t lddt, se_stream_t stream);

/*
 * The same loss on the learned label-embedding table itself (the `labelembeddings` Embedding of
 * learn_labelembedding.py:51-52) instead of a materialised gather of its rows, and the table's gradient.
 *   table [C, C] f32 (ldtab >= C elements between rows); the `tar` row of sample i is
 *   table + clamp(targets[i], 0, C - 1) * ldtab -- the clamp the loss applies to the label everywhere else.
 *   fwd: loss_i and aux are bit for bit those of se_labelembed_loss_fwd on tar = table[clamp(targets)].
 *   bwd: d_out1, d_out2 are bit for bit those of se_labelembed_loss_bwd on that gather; d_table [C, C] (lddtab >= C):
 *        d_table[k, c] = +0, then, for every i with clamp(targets[i]) == k in INCREASING i, one float32 addition of the
 *        value se_labelembed_loss_bwd writes to d_tar[i, c] (wt_i (softmax(table[k])_c - softmax(out2_i / tau)_c),
 *        wt_i = g_i mask_i scale, the same operations and roundings).  Rows with wt_i == 0 are skipped (+0 + +-0 = +0).
 *        Every row of d_table is written; the rows of classes the batch does not contain are +0.  No atomics, no
 *        workspace, no host synchronisation: the bits do not depend on the launch geometry or on concurrent work.
 *        Any of d_out1, d_out2, d_table may be NULL.  B == 0 writes a zero d_table and reads no other array.
 * SE_LABELEMBED_GRID_CAP: most workgroups (of 4 samples each) the per-sample kernels of all four entry points launch;
 *        larger batches stride.
 */
#define SE_LABELEMBED_GRID_CAP 4096
int se_labelembed_table_loss_fwd(const float *out1, int64_t ld1, const float *out2, int64_t ld2,
                                 const float *table, int64_t ldtab, const int64_t *targets, int64_t B,
                                 int64_t C, float tau, float alpha, float beta, float *loss_i, float *aux,
                                 se_stream_t stream);
int se_labelembed_table_loss_bwd(const float *out1, int64_t ld1, const float *out2, int64_t ld2,
                                 const float *table, int64_t ldtab, const int64_t *targets,
                                 const float *grad_loss_i, float grad_scale, int64_t B, int64_t C,
                                 float tau, float alpha, float beta, const float *aux, float *d_out1,
                                 int64_t ldd1, float *d_out2, int64_t ldd2, float *d_table,
                                 int64_t lddtab, se_stream_t stream);

/*
 * DeViSE ranking loss on the class-embedding contraction, forward + backward.
 * Replaces: utils.devise_ranking_loss(embedding, margin)(y_true, y_pred)  (utils.py:103-122)
 *           loss_i = sum_c relu(margin - <y_true_i, y_pred_i> + (y_pred . E^T)[i, c]) - margin
 *           and what TF autodiff derives from it w.r.t. y_pred.
 *   y_pred [B, D] f32; the target rows are E[labels[i]] (labels != NULL, y_true == NULL: the gather of
 *   learn_image_embeddings.py:48-50 done on the device) or the explicit matrix y_true [B, D] (the reference's convention);
 *   emb [C, D] f32; loss_i [B] out.
 *   aux: se_devise_aux_floats(B, C) floats, caller-owned: true_sim [B], active-hinge count [B] and the 0 / 1 hinge mask [B, C]
 *        written by the forward pass and consumed by the backward pass (d y_pred = g_i (mask . E - count_i y_true_i)), followed by
 *        scratch for the forward pass's per-class-slice partial sums when C is large (always ask se_devise_aux_floats for the size).
 *   grad_loss_i [B] or NULL (then every sample uses grad_scale).
 */
int64_t se_devise_aux_floats(int64_t B, int64_t C);
int se_devise_loss_fwd(const float *y_pred, int64_t ldp, const int64_t *labels, const float *y_true, int64_t ldt,
                       const float *emb, int64_t lde, int64_t B, int64_t D, int64_t C, float margin, float *loss_i,
                       float *aux, se_stream_t stream);
int se_devise_loss_bwd(const int64_t *labels, const float *y_true, int64_t ldt, const float *emb, int64_t lde,
                       const float *grad_loss_i, float grad_scale, int64_t B, int64_t D, int64_t C, const float *aux,
                       float *d_pred, int64_t lddp, se_stream_t stream);

/*
 * Center loss (Wen et al.): gradient with respect to the LEARNED class centroids.
 * Replaces: what TF autodiff derives for the `cls_centroids` Embedding of learn_center_loss.py:17-41, whose loss is
 *           center_loss_i = sum_d (x[i, d] - centroids[y_i, d])^2 / 2.  That loss is exactly 0.5 * se_sqdist_loss_fwd, and its
 *           gradient with respect to x is exactly se_sqdist_loss_bwd with the weights w_i / 2: no entry point of their own.
 *   x [B, D] f32 / bf16 (ldx), labels [B] int64 (clamped to [0, C - 1] like the gather of the loss kernels), centroids [C, D] f32 (ldc)
 *   dcent [C, D] f32 out (lddc).  EVERY row is written: dcent[k, d] starts at +0, then acc = acc - fl(w_i * fl(x[i, d] - centroids[k, d]))
 *   runs over the rows i with labels[i] == k in increasing i; w_i = grad_loss_i[i] (NULL: grad_scale for every row).  Rows of
 *   absent classes are +0; B = 0 writes zeros (x and labels may then be NULL).  No atomics, no workspace, no host synchronisation:
 *   the same inputs give the same bits whatever the launch geometry or concurrent work, and the call can be captured in a HIP graph.
 */
int se_center_loss_centroid_grad(const void *x, int x_dtype, int64_t ldx, const int64_t *labels, const float *centroids,
                                 int64_t ldc, const float *grad_loss_i, float grad_scale, int64_t B, int64_t D, int64_t C,
                                 float *dcent, int64_t lddc, se_stream_t stream);

/*
 * Categorical cross-entropy of the softmax classifier on LOGITS, with label smoothing, Keras 2.2's probability clip and the
 * accuracy / top-k metrics of the same scores; forward and backward.
 * Replaces: transform_inputs (learn_classifier.py:17-22: to_categorical + label smoothing on the host), the
 *           'categorical_crossentropy' loss and the 'accuracy' metric of both compile() calls (learn_classifier.py:116-117, 146-147),
 *           utils.top_k_acc (utils.py:49-54), and what TF autodiff derives from the loss with respect to the logits.
 *   logits [B, C] f32 / bf16 (ldz), labels [B] int64 (clamped to [0, C - 1] like the gather of the other loss kernels).
 *   Per row z with label y:  m = max z,  lse = m + log(sum_c exp(z_c - m)),  t_c = lse - z_c  (= -log softmax(z)_c).
 *   Target: Y_c = 1 - s for c == y and s / (C - 1) otherwise when 0 < s < 1 (s = smoothing); one-hot for ANY other s, the reference's
 *   rule.  0 < s < 1 with C < 2 is SE_ERR_INVALID.
 *   Keras 2.2's categorical_crossentropy on a softmax output is -sum_c Y_c log(clip(p_c / sum p, eps, 1 - eps)), eps = float32(1e-7).
 *   In the log domain, with LO = -log(1 - eps) = 1.1920929e-7f and HI = -log(eps) = 16.118095f:
 *       loss_i = sum_c Y_c * min(max(t_c, LO), HI)
 *       a_c    = Y_c where LO <= t_c <= HI, else 0            A_i = sum_c a_c
 *       dz_k   = w_i * (A_i * exp(z_k - lse_i) - a_k)         w_i = grad_loss_i[i] (NULL: grad_scale for every row)
 *   The renormalisation p / sum p is exact in this form (sum p = 1 up to rounding).  The clip caps a sample's loss at HI and gives
 *   ZERO gradient to a class whose probability left [eps, 1 - eps]: with s = 0 a confidently wrong row has loss_i == HI and dz == 0.
 *   t_c is evaluated as (m - z_c) + log(sum): for the arg-max class that is log(sum) itself at full relative precision, so the upper
 *   clip (p > 1 - eps) is decided by the last bit of the float32 sum, as it would be on probabilities; lse - z_c would round t to a
 *   multiple of ulp(lse).  bwd recomputes the forward's t_c bit for bit, so a_k and A_i always agree.
 *   fwd outputs: loss_i [B];  aux: se_softmax_xent_aux_floats(B) = 3 B floats, caller-owned, read by bwd: m_i [B], log(sum)_i [B]
 *        (lse_i = m_i + log(sum)_i, kept apart for the reason above) and A_i [B];
 *        best [B] int32 = arg-max class of the logits, lowest index on ties (np.argmax; Keras' categorical_accuracy is best == y);
 *        above [B] int32 = number of classes whose logit is strictly greater than z_y: tf.nn.in_top_k(k) is above < k (ties in
 *        favour of the target), so one forward pass serves every --top_k_acc;
 *        loss_mean [1] = sum of loss_i / B: thread j of 256 adds loss_i[j], loss_i[j + 256], ... in order, then a binary tree over
 *        the 256 partial sums.  best, above and loss_mean may be NULL.
 *   A row that holds a NaN or +inf: loss_i and its whole dz row are NaN; best is the index of the first NaN, or of the first +inf
 *   if there is no NaN (np.argmax); above = C (never in the top k: TF's rule for a non-finite target score).  -inf logits are legal
 *   (probability 0, clipped); a row of nothing but -inf has no softmax: NaN like a row with a NaN, best = 0.  B = 0 is accepted;
 *   loss_mean is then +0.
 *   bwd: one pass over [B, C]; dz [B, C] f32 / bf16 (lddz).
 *   Asynchronous on `stream`, no allocation, no atomics, no host synchronisation: capturable in a HIP graph, and the same inputs
 *   give the same bits.  Any row pitch; 16-byte loads / stores when pointers and pitches are 16-byte aligned.
 */
int64_t se_softmax_xent_aux_floats(int64_t B);
int se_softmax_xent_fwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, int64_t B, int64_t C,
                        float smoothing, float *loss_i, float *aux, int32_t *best, int32_t *above, float *loss_mean,
                        se_stream_t stream);
int se_softmax_xent_bwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const float *aux,
                        const float *grad_loss_i, float grad_scale, int64_t B, int64_t C, float smoothing, void *dz,
                        int dz_dtype, int64_t lddz, se_stream_t stream);

/*
 * Hierarchy-aware classifier losses on LOGITS: hierarchical cross-entropy (HXE) and cross-entropy against soft labels; forward and
 * backward, with the metrics of se_softmax_xent_fwd.  The reference has neither loss; they are the hierarchy-aware classification
 * baselines of later work.  The weights follow OUR rule (ClassHierarchy.hxe_encoding); no bit parity with any published code is claimed.
 *   logits [B, C] f32 / bf16 (ldz), labels [B] int64 (clamped to [0, C - 1]).  No probability clip in either loss.
 *
 * HXE.  The tree encoding (built on the host, ClassHierarchy.hxe_encoding): pos [C] int32, the position of every class in a
 *   depth-first order of the class tree, so that the classes below any node are one range of positions; path_off [C + 1] int32;
 *   lvl_lo, lvl_hi [nnz] int32 and lvl_w [nnz] float32.  Entries path_off[y] .. path_off[y + 1] are the h_y levels of label y, walking
 *   up: entry l holds the position range [lo, hi) of the l + 1-th ancestor a_{l+1} (a_0 = y; the last range is [0, C)) and the weight
 *   lambda_l of the edge a_l -> a_{l+1}.  Ranges grow strictly along a path (the host drops levels that add no class) and
 *   h_y <= SE_HXE_MAX_LEVELS.  path_off_host is the SAME array in HOST memory: the entry points check it before any launch (starts at
 *   0, every h_y in [0, SE_HXE_MAX_LEVELS]; anything else is SE_ERR_INVALID) and take nnz from it; the kernels read the device copy.
 *   Per row z with label y:  M = max z,  e_c = exp(z_c - M),  L_0 = z_y - M (exact: no exp / log round trip),
 *       S_{l+1} = sum of e_c over lo_l <= pos[c] < hi_l        L_{l+1} = max(log S_{l+1}, L_0)
 *       loss_i  = sum_{l = 0}^{h - 1} lambda_l * (L_{l+1} - L_l)        (a term whose two logs are equal, -inf included, is 0)
 *   Mathematically S_{l+1} >= e_y, so the floor at L_0 only acts when a whole range underflows in float32; the loss then stays finite,
 *   and where the floor acts the term is a BOUND of the exact value, not the exact value.
 *   With lev(c) the smallest k such that c lies in R_k (R_0 = {y}, R_k = range k - 1), r_k = 1 / S_k (0 where S_k == 0), lambda_h = 0:
 *       H_k  = sum_{j = max(k, 1)}^{h} (lambda_{j-1} - lambda_j) * r_j     (= sum_{l >= k-1} lambda_l / S_{l+1} - sum_{l >= max(k,1)} lambda_l / S_l)
 *       dz_c = w_i * e_c * H_lev(c)   (c != y)          dz_y = w_i * (e_y * H_0 - lambda_0)
 *   The label's own l = 0 term is the constant -lambda_0, never e_y / S_0.  With every lambda = 1 this is p - onehot; the exact sum of
 *   a row's gradients is 0.  aux: se_hxe_aux_floats(B) = (2 + SE_HXE_MAX_LEVELS) B floats, row i at aux + (2 + SE_HXE_MAX_LEVELS) i:
 *   M_i, then H_0 .. H_h (the rest unused), so that bwd is ONE pass over [B, C].
 *
 * Soft labels.  table [C, C] float32 (ldt): row y is the target distribution Q[y, :] (ClassHierarchy.soft_label_table).
 *       loss_i = sum_c Q[y,c] * ((M - z_c) + log S),  evaluated as  sum_c Q[y,c] (M - z_c)  +  (sum_c Q[y,c]) * log S,   S = sum_c e_c
 *       dz_k   = w_i * ((sum_c Q[y,c]) * p_k - Q[y,k])        p_k = exp(-((M - z_k) + log S))
 *   A class with Q[y,c] == 0 contributes nothing, whatever its logit.  aux: 3 B floats (M [B], log S [B], sum_c Q[y,c] [B]).
 *
 * All four: best, above, loss_mean and the rules for rows with a NaN or +inf or nothing but -inf are those of se_softmax_xent_fwd
 *   (the same row code); best, above and loss_mean may be NULL.  w_i = grad_loss_i[i] (NULL: grad_scale for every row).  Every C that
 *   se_softmax_xent_fwd accepts; B = 0 is accepted.  Any row pitch; 16-byte loads / stores when pointers and pitches are 16-byte
 *   aligned.  A wave per row up to C = 1024, a workgroup per row above; each row is read twice (the second read hits the cache).
 *   Asynchronous on `stream`, no allocation, no atomics, no host synchronisation: capturable in a HIP graph.  Every reduction runs in
 *   a fixed order: the same inputs give the same bits, and a row's bits depend neither on B nor on the other rows.
 */
#define SE_HXE_MAX_LEVELS 32
int64_t se_hxe_aux_floats(int64_t B);
int se_hxe_fwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const int32_t *pos, const int32_t *path_off,
               const int32_t *path_off_host, const int32_t *lvl_lo, const int32_t *lvl_hi, const float *lvl_w, int64_t B, int64_t C,
               float *loss_i, float *aux, int32_t *best, int32_t *above, float *loss_mean, se_stream_t stream);
int se_hxe_bwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const int32_t *pos, const int32_t *path_off,
               const int32_t *path_off_host, const int32_t *lvl_lo, const int32_t *lvl_hi, const float *lvl_w, const float *aux,
               const float *grad_loss_i, float grad_scale, int64_t B, int64_t C, void *dz, int dz_dtype, int64_t lddz,
               se_stream_t stream);
int se_soft_xent_fwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const float *table, int64_t ldt, int64_t B,
                     int64_t C, float *loss_i, float *aux, int32_t *best, int32_t *above, float *loss_mean, se_stream_t stream);
int se_soft_xent_bwd(const void *logits, int z_dtype, int64_t ldz, const int64_t *labels, const float *table, int64_t ldt,
                     const float *aux, const float *grad_loss_i, float grad_scale, int64_t B, int64_t C, void *dz, int dz_dtype,
                     int64_t lddz, se_stream_t stream);

/*
 * Conditional risk minimisation (CRM) on a class TREE: the expected LCS height of every class under a row of class probabilities, and
 * the `top` classes of smallest risk -- the inference-time baseline of the hierarchy-aware losses above (predict the class k that
 * minimises sum_j p_j * height(lcs(k, j)) instead of the arg-max of p).  The reference has no such decoding.  The dense form is
 * P @ H^T with the [C, C] height table, O(C^2) per row; on a tree it is O(C * levels):
 *   probs [N, C] float32 (ldp).  pos, path_off, lvl_lo, lvl_hi: exactly what se_hxe_fwd reads (ClassHierarchy.tree_risk_encoding builds
 *   them with the heights): entries path_off[k] .. path_off[k + 1] are the levels of class k walking up, entry e the position range
 *   [lo, hi) of an ancestor; the ranges of a path are nested and grow strictly, the last one is [0, C), at most SE_HXE_MAX_LEVELS of
 *   them.  lvl_h [nnz] int32: the height (an integer >= 0) of the node whose range entry e holds; own_h [C] int32: the height of
 *   class k itself (NULL: all 0).  No host copy of path_off is needed: the kernel clamps what it reads (below).
 *   Per row, with the float32 inputs widened to float64:  q[pos[c]] = p[c];  the mass of a range is the sum of q over it;
 *       risk_k = own_h[k] * p_k + sum_{l = 0}^{h_k - 1} lvl_h[l] * (m_l - m_{l-1}),    m_{-1} = p_k,   m_l = mass of range l of k
 *   (the classes whose lowest common subsumer with k is the level-l ancestor are that ancestor's range minus the range below it).
 *   Every mass is a difference of two entries of ONE float64 prefix sum of q.  The order of its additions is a function of C alone:
 *   a row's bits depend neither on N nor on the row's place in the batch nor on the launch geometry.
 *   out_cls [N, top] int32: the `top` classes in ascending (risk, class index) order, the float64 risks compared as numbers
 *   (-0 == +0, NaN last); out_risk [N, top] float64: their risks; risk [N, C] float64 (ldr) or NULL: all C values.  The lists are the
 *   same bits whether or not risk is requested.
 *   A row that holds a NaN or an infinity gets NaN for every risk and the classes 0 .. top - 1 (an explicit rule: otherwise the result
 *   would depend on whether a mass is summed directly or taken as a difference of prefixes).
 *   No gather leaves its table, whatever the device tables hold: pos is clamped into [0, C), lo / hi into [0, C] (hi <= lo: an empty
 *   range), the level count of a path to min(SE_HXE_MAX_LEVELS, nnz) and its start into [0, nnz - levels].
 *   SE_ERR_INVALID: a NULL required pointer, ldp < C, risk && ldr < C, top outside [1, min(C, SE_TREE_RISK_TOP_MAX)], C < 1, N < 0,
 *   nnz < 0.  SE_ERR_UNSUPPORTED: C > SE_TREE_RISK_MAX_CLASSES (the prefix sums and the risks of a row in flight, two float64 rows,
 *   live in the 160 KiB LDS).  N == 0 returns SE_OK without a launch.
 *   A wave per row up to C = 1024, a workgroup per row above; any row pitch and alignment.  Asynchronous on `stream`, no allocation, no
 *   workspace, no atomics, no host synchronisation: capturable in a HIP graph.
 */
#define SE_TREE_RISK_TOP_MAX 32
#define SE_TREE_RISK_MAX_CLASSES 10000
int se_tree_risk_topk(const float *probs, int64_t ldp, const int32_t *pos, const int32_t *path_off, const int32_t *lvl_lo,
                      const int32_t *lvl_hi, const int32_t *lvl_h, int nnz, const int32_t *own_h, int64_t N, int C, int top,
                      int32_t *out_cls, double *out_risk, double *risk, int64_t ldr, se_stream_t stream);

/*
 * Adagrad update of a flat float32 parameter buffer in one launch, gradient scale and L2 regulariser folded in.
 * Replaces: Keras 2.2 optimizers.Adagrad.get_updates [third party, not in the reference tree] as learn_devise.py:87,114 uses it
 *           (keras.optimizers.Adagrad(lr=...) in both compile() calls), and the whole-buffer passes that would otherwise scale the
 *           gradient (the mean over the data-parallel ranks) and add the kernel regulariser's gradient in front of it.
 *   p [n] in / out, accum [n] in / out (the running sum of squared gradients, zeros before the first step), g [n] in,
 *   l2 [n] or NULL: the coefficient 2 lambda of every element (0 where a parameter has no regulariser).
 *   Per element, every operation a separately rounded float32 operation (no FMA contraction; correctly rounded division and square root):
 *       g1 = grad_scale == 1 ? g : g * grad_scale
 *       g2 = l2 ? g1 + l2 * p : g1
 *       a' = a + g2 * g2
 *       p' = p - (lr * g2) / (sqrt(a') + epsilon)             Keras: p - lr * g / (K.sqrt(new_a) + epsilon)
 *   lr_dev NULL: the learning rate is the argument lr; otherwise it is read from lr_dev[0] on the device when the kernel runs (lr
 *   is then ignored), so a captured launch follows a schedule without being captured again.
 *   g is ONLY READ: after the step it still holds the raw gradient, neither scaled nor regularised.
 *   An element with g2 = 0 keeps p and accum bit for bit when epsilon > 0 (+0 stays +0); a NaN or Inf in g makes p and accum of that element NaN or
 *   Inf as the formula says: it is not an error.
 *   n = 0 returns SE_OK without a launch (every pointer may then be NULL); n < 0, epsilon < 0 or NaN, or a NULL p / accum / g with
 *   n > 0 is SE_ERR_INVALID.  Any pointer alignment and any n: 16-byte accesses when p, accum, g and l2 are all 16-byte aligned, with
 *   the n % 4 last elements taken one by one; 4-byte accesses otherwise.  int64 indices.  The grid is capped at
 *   SE_ADAGRAD_MAX_BLOCKS workgroups of 256 threads that stride over the buffer.
 *   Asynchronous on `stream`, no allocation, no atomics, no host synchronisation: capturable in a HIP graph, and the same inputs
 *   give the same bits.
 */
#define SE_ADAGRAD_MAX_BLOCKS 2048
int se_adagrad_step(float *p, float *accum, const float *g, const float *l2, int64_t n, float lr, const float *lr_dev,
                    float grad_scale, float epsilon, se_stream_t stream);

/*
 * Keras 2.2 SGD on a flat float32 parameter buffer with a deterministic global-norm clip: the norm and clip factor of the
 * regularised gradient (se_grad_clip_factor: one launch over the buffers and a one-wave finalising launch), then the whole update in
 * one launch (se_sgd_step) -- gradient scale, L2 regulariser, clip factor, learning rate, momentum and Nesterov folded in.
 * Replaces: Keras 2.2 optimizers.SGD.get_updates with clipnorm [third party, not in the reference tree] as every trainer of
 *           learn_image_embeddings.py / learn_classifier.py / learn_center_loss.py / learn_labelembedding.py compiles it
 *           (keras.optimizers.SGD(lr=..., momentum=0.9, nesterov=..., clipnorm=args.clipgrad)), and the whole-buffer passes that
 *           otherwise scale the gradient, add the regulariser's, take the norm, clip, and apply velocity and weights one by one.
 *   Common to both: g [n] in, ONLY READ (after the calls it still holds the raw gradient, neither scaled, regularised nor clipped);
 *   l2 [n] or NULL: the coefficient 2 lambda of every element; per element, every operation a separately rounded float32 operation
 *   (no FMA contraction; correctly rounded division):
 *       g1 = grad_scale == 1 ? g : g * grad_scale
 *       g2 = l2 ? g1 + l2 * p : g1
 *   Any pointer alignment and any n: 16-byte accesses when every buffer of the call is 16-byte aligned (the n % 4 last elements
 *   are taken one by one), 4-byte accesses otherwise; int64 indices; grids capped at SE_SGD_MAX_BLOCKS workgroups of 256 threads
 *   that stride over the buffers.  Asynchronous on `stream`, no allocation, no atomics, no host synchronisation: capturable in a
 *   HIP graph, and the same inputs give the same bits.
 *
 * se_grad_clip_factor: stats[0] = norm = (float)sqrt(S), S = sum of (double)g2 * (double)g2 in float64 (a float32 square is exact
 *   in float64); stats[1] = factor = min(clipnorm / (norm + 1e-12f), 1.0f) with a float32 sum and a float32 quotient, NaN for a
 *   NaN norm (and 0 for an infinite one): the value of torch.clamp(clipnorm / (norm + 1e-12), max=1.0).
 *   p [n] may be NULL when l2 is.  workspace: se_grad_clip_workspace_bytes() bytes of device memory, 8-byte aligned; its contents
 *   before the call do not matter and nothing is kept in it between calls.  stats: 2 floats of device memory.
 *   The order of the additions is fixed by n and the alignment class (16-byte or not) alone: thread t of workgroup b adds its
 *   elements in ascending order (four per 16-byte unit; the n % 4 tail elements go to threads 0 .. 2 of workgroup 0, behind their units), the 64 lanes
 *   of a wave are summed by one xor butterfly (offsets 32, 16, ... 1), the four waves in order, and each workgroup writes its float64
 *   partial to workspace[b]; the finalising wave adds partials lane, lane + 64, ... in ascending order and its lanes by the same
 *   butterfly.  No floating-point atomics.
 *   n = 0 returns SE_OK without a launch and leaves stats alone; n < 0, a clipnorm that is not finite and > 0, a NULL g /
 *   workspace / stats with n > 0, a workspace that is not 8-byte aligned, or l2 without p is SE_ERR_INVALID.
 *
 * se_sgd_step: p [n] in / out, v [n] in / out (the velocity, zeros before the first step).  Per element, each operation rounded:
 *       g3   = clip_dev ? g2 * clip_dev[0] : g2               clip_dev = &stats[1] of se_grad_clip_factor
 *       step = lr * g3
 *       v'   = momentum * v - step                            Keras: v = self.momentum * m - lr * g
 *       p'   = nesterov ? (p + momentum * v') - step          Keras: p + self.momentum * v - lr * g
 *                       : p + v'
 *   lr_dev NULL: the learning rate is the argument lr; otherwise it is read from lr_dev[0] on the device when the kernel runs (lr
 *   is then ignored), as clip_dev[0] is, so a captured launch follows a schedule without being captured again.
 *   Words that are +0 in p, v, g and l2 stay +0 in p and v (for a finite factor and learning rate); a NaN or Inf in g, or a NaN
 *   factor, spreads as the formula says: it is not an error.
 *   n = 0 returns SE_OK without a launch (every pointer may then be NULL); n < 0, a momentum < 0 or NaN, or a NULL p / v / g with
 *   n > 0 is SE_ERR_INVALID.
 */
#define SE_SGD_MAX_BLOCKS 2048
size_t se_grad_clip_workspace_bytes(void);
int se_grad_clip_factor(const float *g, const float *p, const float *l2, int64_t n, float grad_scale, float clipnorm,
                        void *workspace, float *stats, se_stream_t stream);
int se_sgd_step(float *p, float *v, const float *g, const float *l2, int64_t n, float lr, const float *lr_dev,
                float grad_scale, const float *clip_dev, float momentum, int nesterov, se_stream_t stream);

/*
 * The pyramidal residual shortcut in one launch, and the gradient of its pooled operand:
 *     out = s + ChannelPadding((pad_before, C - Cin - pad_before))(AveragePooling2D(stride)(x))
 * Replaces: layers.add([s, shortcut(x, n, stride)]) at the end of every block of models/cifar_pyramidnet.py:81-110 (pad_before = 0)
 *           and the same composition of models/cifar_resnet.py:28-147 (symmetric padding: pad_before = (C - Cin) / 2), which as
 *           pooling + padding + add write a zero-padded copy of the shortcut as large as s only for the add to read it again.
 *   s, out  [B, C, H, W] logical;  x [B, Cin, Hx, Wx] logical, Cin + pad_before <= C
 *   stride  1 (H == Hx, W == Wx) or 2 (H == Hx / 2, W == Wx / 2 rounded down: a trailing odd row or column of x belongs to no
 *           window, as in Keras' 'valid' pooling and torch's floor mode); any other stride is SE_ERR_UNSUPPORTED
 *   layout  SE_LAYOUT_NCHW: all tensors dense in the order [B, C, H, W];  SE_LAYOUT_NHWC: dense in the order [B, H, W, C]
 *           (torch's channels_last).  Operands and output share it.
 *   dtype   SE_DTYPE_F32 or SE_DTYPE_BF16; operands and output share it
 * Forward, per element, in float32 with every operation separately rounded (no contraction); bf16 values are widened first:
 *   channel c in [pad_before, pad_before + Cin), ci = c - pad_before:
 *       acc    = the window's stride * stride values x[b, ci, stride h + i, stride w + j] added one by one in row-major window order
 *                (i outer, j inner), starting from the first:  ((x00 + x01) + x10) + x11
 *       pooled = acc / (float)(stride * stride)
 *       out    = s + pooled, rounded once to the output dtype (bf16: to nearest even)
 *   every other channel: out = s, the BITS copied (not "s + 0.0f"): -0.0 and NaN payloads pass through.
 *   out may be s itself (every element is read before it is written, by the same thread); it must not overlap x.
 * Backward (se_shortcut_add_bwd), dout [B, C, H, W] and dx [B, Cin, Hx, Wx] in the same layout and dtype:
 *       dx[b, ci, y, x] = dout[b, pad_before + ci, y / stride, x / stride] / (float)(stride * stride), rounded to the dtype;
 *       +0 at the positions of a trailing odd row or column.
 *   The gradient of s is dout itself: there is no kernel for it.  Windows do not overlap, so every dx element has one source.
 * One launch each, asynchronous on `stream`; no workspace, no allocation, no atomics, no host synchronisation: capturable in a HIP
 * graph, and the same inputs give the same bits.  Any channel count and image size: accesses are as wide (up to 16 bytes) as the
 * extents and the pointers' alignment allow, element by element otherwise.  int64 offsets; the grid is capped at
 * SE_SHORTCUT_MAX_BLOCKS workgroups of 256 threads that stride over the tensor.
 * B == 0 (or any empty tensor) returns SE_OK without a launch, whatever the pointers.  A bad dtype or layout code, a negative
 * extent, Cin + pad_before > C, H or W that do not follow from Hx, Wx and stride, or a NULL pointer to a non-empty tensor is
 * SE_ERR_INVALID.  Every argument is checked before any device work.
 */
#define SE_LAYOUT_NCHW 0
#define SE_LAYOUT_NHWC 1
#define SE_SHORTCUT_MAX_BLOCKS 2048
int se_shortcut_add_fwd(const void *s, const void *x, void *out, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W,
                        int64_t Cin, int64_t Hx, int64_t Wx, int stride, int64_t pad_before, se_stream_t stream);
int se_shortcut_add_bwd(const void *dout, void *dx, int dtype, int layout, int64_t B, int64_t C, int64_t H, int64_t W, int64_t Cin,
                        int64_t Hx, int64_t Wx, int stride, int64_t pad_before, se_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Retrieval side  (evaluate_retrieval.pairwise_retrieval, evaluate_retrieval.py:22-73)
 * ------------------------------------------------------------------------------------------ */

/* sq[i] = float32 np.sum(x[i]**2)  with NumPy's pairwise summation order, bit-exact.
 * Replaces: `sqnorm = np.sum(features ** 2, axis = -1)`          evaluate_retrieval.py:61 */
int se_row_sqnorm(const float *x, int64_t ldx, int64_t n, int64_t d, float *sq, se_stream_t stream);

/* x[i] /= sqrt(np.sum(x[i]*x[i]))  in place, bit-exact w.r.t. float32 NumPy.
 * Replaces: `features /= np.linalg.norm(features, axis = -1, keepdims = True)`
 *                                                                 evaluate_retrieval.py:58 */
int se_normalize_rows(float *x, int64_t ldx, int64_t n, int64_t d, se_stream_t stream);

/*
 * All-pairs distance matrix  out[i, j] = dist(a[i], b[j]),  i < q, j < n.
 * Replaces: `pdist = -np.dot(features, features.T)`               evaluate_retrieval.py:59
 *           `pdist = ne.evaluate('A + B - 2 * C', ...)`           evaluate_retrieval.py:61-62
 * The dot product is a sequential fp32 FMA chain over k = 0..d-1 (v_mfma_f32_32x32x2_f32),
 * bit-identical to the OpenBLAS sgemm/ssyrk result the reference obtains for d <= 448.
 * kblocks (HOST pointer, may be NULL): K-block lengths summing to d; the chain restarts from 0
 * at each block and block results are added in order (OpenBLAS behaviour for large d).
 *   sqa [q], sqb [n]: row square norms, required for SE_METRIC_EUCLID only.
 */
int se_pairwise_dist(const float *a, int64_t lda, const float *b, int64_t ldb, const float *sqa,
                     const float *sqb, int64_t q, int64_t n, int64_t d, int metric,
                     const int32_t *kblocks, int nkb, float *out, int64_t ldo,
                     se_stream_t stream);

/*
 * Full ranking of every row:  rank[i, r] = column index of the r-th smallest pdist[i, :]
 * under the canonical order (distance ascending, index ascending; NaN last; -0 == +0).
 * Replaces: `ranking = np.argsort(pdist, axis = -1)`              evaluate_retrieval.py:67
 * (the reference's sort is unstable: ties are returned in canonical order here).
 *   rank: int32 [q, n] when idx64 == 0, int64 [q, n] (NumPy's dtype) when idx64 == 1, uint16 [q, n] when idx64 == 2 (rows of at
 *   most 53,248 columns only -- SE_ERR_UNSUPPORTED otherwise: the width the register-resident kernel holds its ranks in; half the
 *   bytes for se_hierarchical_precision_r16 to read).  ldr in elements of that type.
 *   workspace: se_rank_rows_workspace_bytes(q, n) bytes of device memory, 16-byte aligned.  n <= 53,248: one workgroup sorts a row in registers
 *   (4.4 KB of workspace: probe / guard words); 53,248 < n <= 425,984: 2, 4 or 8 segments of a row are sorted the same way into
 *   runs and merged pairwise (merge tree; up to 3 GB of run planes / level buffers for a chunk of rows at a time); longer rows:
 *   LDS-tiled radix sort through 16 bytes per key of scratch per resident workgroup.
 */
int64_t se_rank_rows_workspace_bytes(int64_t q, int64_t n);
int se_rank_rows(const float *pdist, int64_t ldp, int64_t q, int64_t n, void *rank, int idx64,
                 int64_t ldr, void *workspace, int64_t workspace_bytes, se_stream_t stream);

/*
 * One-time set-up of the ranking on the CURRENT device -- the only entry point of the ranking that synchronises by design.
 * The fastest kernels of se_rank_rows take their stable order from the lane order in which the LDS serves same-address
 * returning adds of one wave instruction: gfx950 serves them in ascending lane order, the ISA does not promise it.  This call
 * (1) probes the property (64 workgroups, four conflict patterns, the production counter format) and (2) ranks crafted
 * tie-heavy rows through EVERY hardware-ordered kernel variant (short / long instantiation x plain / group-peeling / two-pass,
 * segment runs + merge) and audits every row of every result (se_rank_rows_check's kernel).  The verdict is cached per device:
 * afterwards se_rank_rows is purely asynchronous -- no probe, no guard, no host round trip; it can be captured into a HIP graph --
 * and uses the hardware-ordered kernels iff both steps passed (else the ballot / tiled kernels, whose order holds by construction).
 * WITHOUT this call the first se_rank_rows of a process on a device does the probe itself and audits 512 sampled rows of its own
 * result (hipStreamSynchronize + one 4-byte copy, ~0.5 ms) before it returns; a call that cannot (no workspace for the guard, or
 * a stream under capture) uses the ballot kernel.
 *   workspace: se_rank_rows_init_workspace_bytes() bytes (~5 MB), 256-byte aligned; may be freed afterwards.  ~3 ms.
 */
int64_t se_rank_rows_init_workspace_bytes(void);
int se_rank_rows_init(void *workspace, int64_t workspace_bytes, se_stream_t stream);

/*
 * Order guard of se_rank_rows: counts the rows of a finished ranking that violate the canonical order -- along every row
 * (pdist[rank[r]], rank[r]) must precede (pdist[rank[r + 1]], rank[r + 1]), every index lies in [0, n).  One gather of the
 * distances through the ranks (random 4-byte reads: ~1 us per row of 50k columns).  se_rank_rows runs the same check by
 * itself -- on 512 evenly spaced rows behind the first ranking a process does with its fastest kernel (whose stable order rests
 * on a hardware property the library can probe but the ISA does not promise), on every row of every call when SE_RANK_CHECK=1
 * is set -- and re-ranks with the guaranteed-order kernel when it finds a violation; this entry point lets a caller audit any
 * ranking in full (np.argsort(pdist, axis=-1, kind='stable') passes it).
 *   idx64: index width code of the ranking, as for se_rank_rows: 0 = int32, 1 = int64, 2 = uint16 (n <= 65536 only).
 *   workspace: se_rank_rows_check_workspace_bytes() bytes; *bad_rows_host (HOST pointer) receives the count; synchronises.
 */
int64_t se_rank_rows_check_workspace_bytes(void);
int se_rank_rows_check(const float *pdist, int64_t ldp, int64_t q, int64_t n, const void *rank, int idx64,
                       int64_t ldr, void *workspace, int64_t workspace_bytes, int64_t *bad_rows_host,
                       se_stream_t stream);

/*
 * Float64 retrieval (opt-in: float64 feature files, whose distances the reference computes and ranks in float64).
 *
 * se_pairwise_dist_f64: all-pairs distance matrix of float64 operands, out[i, j] = dist(a[i], b[j]), i < q, j < n.
 * Replaces: `pdist = -np.dot(features, features.T)`               evaluate_retrieval.py:59   for float64 features
 *           `pdist = ne.evaluate('A + B - 2 * C', ...)`           evaluate_retrieval.py:61-62
 * Canonical float64 arithmetic, held bit for bit (NaN payloads aside):
 *   C[i, j]   = the sequential float64 FMA chain acc = fma(a[i, k], b[j, k], acc), k = 0 .. d - 1 ascending, from acc = +0.0
 *               (v_fma_f64; ONE chain: there are no K blocks -- the float64 BLAS of the host follows no rule that could be pinned,
 *               DESIGN.md section 3.1);
 *   cosine    out = -C;
 *   Euclidean out = (sqa[i] + sqb[j]) - 2 * C: one addition and one subtraction, each rounded on its own (no contraction; 2 * C is
 *               exact) -- numexpr's left-to-right evaluation of 'A + B - 2 * C'.
 *   a [q, d], b [n, d] float64 (lda, ldb); sqa [q], sqb [n] float64 row square norms, required for SE_METRIC_EUCLID only (the
 *   caller computes them -- and normalises rows for the cosine metric -- with the reference's own NumPy lines on the host);
 *   metric: SE_METRIC_COSINE or SE_METRIC_EUCLID; out [q, n] float64 (ldo);
 *   img [q, n] float32 (ldi) or NULL: img = (float)out, rounded to nearest even.  The cast is monotone non-decreasing, so the
 *   canonical ranking of img (se_rank_rows) orders every pair of columns with different images as out does.
 *   q == 0 or n == 0 returns SE_OK without a launch; d == 0 gives the distances of empty dot products.  Asynchronous on `stream`,
 *   no workspace, no atomics.
 *
 * se_rank_refine_f64: turns rank = se_rank_rows(img) into the canonical ranking of out64 itself -- (float64 distance, index)
 * ascending, NaN last, -0.0 == +0.0, equal values index-ascending: `np.argsort(pdist, axis = -1)` of float64 distances
 * (evaluate_retrieval.py:67) with ties in canonical order.  Per row, every maximal run of adjacent ranks whose images are equal
 * (==: +-0 are one run, the NaNs are one run) is sorted in place by (float64 canonical key, index); ranks outside such runs are
 * not touched.  Runs of any length up to n: up to 8 ranks in one thread's registers, up to 1,024 from LDS, longer ones by a
 * second launch from the workspace (chunks of 1,024 sorted from LDS, then ranked against each other by binary search).  The result does not rest on the lane-order property that
 * se_rank_rows_init probes.
 *   out64 [q, n] float64 (ld64), img [q, n] float32 (ldi): as written by se_pairwise_dist_f64 (any matrix pair with
 *   img = (float)out64 will do); rank [q, n] in / out: int32 when idx64 == 0, int64 when idx64 == 1 (ldr in elements);
 *   idx64 == 2 (uint16) is SE_ERR_UNSUPPORTED.  Indices outside [0, n) are read as 0 (no gather leaves its row).
 *   workspace: se_rank_refine_f64_workspace_bytes(q, n) bytes of device memory, 16-byte aligned; its contents before the call do
 *   not matter.  Asynchronous on `stream`, no allocation, no atomics, no host synchronisation: capturable in a HIP graph.
 */
int se_pairwise_dist_f64(const double *a, int64_t lda, const double *b, int64_t ldb, const double *sqa,
                         const double *sqb, int64_t q, int64_t n, int64_t d, int metric, double *out,
                         int64_t ldo, float *img, int64_t ldi, se_stream_t stream);
int64_t se_rank_refine_f64_workspace_bytes(int64_t q, int64_t n);
int se_rank_refine_f64(const double *out64, int64_t ld64, const float *img, int64_t ldi, int64_t q, int64_t n,
                       void *rank, int idx64, int64_t ldr, void *workspace, int64_t workspace_bytes,
                       se_stream_t stream);

/*
 * The k nearest columns of every row of a distance matrix, canonical order, with a global
 * column offset (sharded galleries: shard r passes col_offset = first gallery row of the shard).
 *   out_d [q, k] f32, out_i [q, k] int32 (global indices).  k <= n, k <= SE_TOPK_MAX.
 */
#define SE_TOPK_MAX 2048
int se_topk_rows(const float *pdist, int64_t ldp, int64_t q, int64_t n, int64_t col_offset, int k,
                 float *out_d, int32_t *out_i, se_stream_t stream);

/*
 * Merge per-shard top-k lists (e.g. the RCCL all-gather of every rank's se_topk_rows output)
 * into the global top-k; the result is independent of how the gallery was sharded.
 *   d, idx: [parts, q, k];  out_d, out_i: [q, k].  parts * k <= SE_TOPK_MAX * 4.
 *   Lists as se_retrieve_topk / se_topk_rows write them (ascending under the canonical (distance, index) order) merge fastest
 *   (k <= 1024: one wave per query, the running best list in registers); a list that is not ascending is sorted first -- same result.
 */
int se_topk_merge(const float *d, const int32_t *idx, int parts, int64_t q, int k, float *out_d,
                  int32_t *out_i, se_stream_t stream);

/*
 * The same merge on PACKED lists: part p is one contiguous block of 2 q k 32-bit words -- its [q, k] distances (f32) followed by
 * its [q, k] indices (i32).  That is the receive buffer of ONE all-gather in which every rank contributes its (dist | idx) block
 * (sharded_retrieval.all_gather_lists): half the collectives of gathering distances and indices separately.
 */
int se_topk_merge_packed(const void *packed, int parts, int64_t q, int k, float *out_d, int32_t *out_i,
                         se_stream_t stream);

/*
 * Fused distance + top-k: the k nearest gallery rows of every query WITHOUT the [q, n] distance matrix
 * (SURVEY.md section 8d "fused top-k": bytes = 4 (q + n) d + 8 q k).
 * Replaces: the head of evaluate_retrieval.py:57-67 (normalise / distances / np.argsort) for consumers that read only the
 *           first k entries of every ranking (P@k and clipped AHP without AP, class_hierarchy.py:300-309), and it is the
 *           per-shard step of the sharded-gallery split (gallery shard r passes col_offset = its first global row).
 * Same arithmetic as se_pairwise_dist (sequential fp32 FMA chain, optional K-block list `kblocks` -- HOST pointer, may be
 * NULL -- for d > 448, evaluate_retrieval.py:59 on OpenBLAS) and the same canonical order as se_rank_rows: out_i[i, :] ==
 * the first k entries of se_rank_rows(se_pairwise_dist(queries, gallery))[i], out_d the distances, bit for bit.
 * Galleries of >= 16384 rows (k <= 512): the Q x N distances are first BOUNDED, not computed -- a pass on the fp16 matrix cores
 * (v_mfma_f32_32x32x16_f16) over half-precision IMAGES of the operands (each matrix scaled by one power of two so that its largest
 * entry sits just below 2^14, entries below fp16's normal range flushed to zero, columns padded to a multiple of 128) gives d~
 * with |d~ - d| <= eps(query) (a rigorous bound from the operands' actual rounding residuals).  A sample of <= 4096 gallery rows gives every query a threshold, the full pass appends the few
 * items with d~ <= threshold to per-query candidate lists, and a per-query kernel recomputes, with the exact fp32 chain, the items
 * within 2 eps of the list's k-th smallest d~, sorts them and accepts the first k once it has proved that nothing outside that set
 * can precede them; queries it cannot prove (short / overflowing lists, NaN rows, tie groups of thousands) are redone exactly over the
 * whole gallery.  The output does not depend on what the half-precision pass computed.  Smaller galleries go through a [rows, n] distance slab
 * in the workspace; k > 512 through the fp32 form of the same passes.
 *   metric: SE_METRIC_COSINE or SE_METRIC_EUCLID (then sqq [q], sqg [n] = se_row_sqnorm of the operands).
 *   workspace: se_retrieve_topk_workspace_bytes(q, n, d, ldg, k) bytes, 256-byte aligned -- the ONLY supported way to size it (it
 *   holds the candidate sub-lists, the fp16 images at 2 bytes x (n + q) x (d rounded up to a multiple of 128), per-row norms and
 *   bounds, and the scratch rows of the exact fallback; the split between them follows the pass geometry chosen for (q, n, d)).
 */
int64_t se_retrieve_topk_workspace_bytes(int64_t q, int64_t n, int64_t d, int64_t ldg, int k);
int se_retrieve_topk(const float *queries, int64_t ldq, const float *gallery, int64_t ldg,
                     const float *sqq, const float *sqg, int64_t q, int64_t n, int64_t d,
                     int metric, const int32_t *kblocks, int nkb, int64_t col_offset, int k,
                     float *out_d, int32_t *out_i, void *workspace, int64_t workspace_bytes,
                     se_stream_t stream);

/*
 * k-nearest-neighbour classification: the vote over every query's neighbour list (a consumer of se_retrieve_topk / se_topk_merge).
 * Replaces: sklearn.neighbors.KNeighborsClassifier(n_neighbors = k, weights = 'uniform', algorithm = 'brute') -- the counts behind
 *           predict_proba and the smallest-label-among-ties rule of predict -- on neighbour lists that are already there (the
 *           reference has no k-NN line), for several k and the `top` best classes at once.
 *   idx       [q, list_len] int32 global gallery indices, best first (ldi elements between rows); 1 <= list_len <= SE_TOPK_MAX
 *   cls       [gallery] int32 class index of every gallery item
 *   qidx      [q] int32 gallery index of the query itself, or NULL
 *   ks        [nk] int32 cut-offs, HOST pointer (read before the launch): strictly ascending, each in [1, list_len];
 *             nk <= SE_KNN_KS_MAX (more is SE_ERR_UNSUPPORTED)
 *   top       classes to report per (query, cut-off): 1 .. SE_KNN_TOP_MAX and <= num_classes
 *   out_cls, out_votes   [q, nk, top] int32
 * Who votes: the list is walked in order.  An entry outside [0, gallery) -- the 2^31 - 1 pads of short shards, -1 -- is skipped (no
 * gather leaves cls), and so is an entry equal to qidx[i] (leave-one-out).  Every other entry is one of the query's NEIGHBOURS and
 * votes for class cls[entry] with weight 1; a class value outside [0, num_classes) casts no vote but still counts as a neighbour.
 * For cut-off ks[j] the first ks[j] neighbours vote -- all of them when the list holds fewer (a list of exactly ks[j] entries that
 * contains the query, or pads).
 * Ranking: out_cls[i, j, :] = the `top` best classes under (votes descending, class index ascending), out_votes their vote counts;
 * classes without a vote fill the tail in ascending class index with 0 votes.  The tie rule is that of se_rank_rows on negated
 * scores and of scikit-learn's uniform-weight predict.
 *   Everything is an integer: the same inputs give the same bits on every launch geometry.  num_classes is not limited (the
 *   per-query vote table has 2 * list_len slots, whatever the number of classes).  q == 0 or nk == 0 returns SE_OK without a launch.
 *   SE_ERR_INVALID: a NULL idx / cls / ks / out_cls / out_votes, ldi < list_len, list_len outside [1, SE_TOPK_MAX], top out of range,
 *   cut-offs that do not ascend or leave [1, list_len], num_classes < 1, a negative size.
 *   Asynchronous on `stream`; no workspace, no allocation, no host synchronisation, no float atomics: capturable in a HIP graph.
 */
#define SE_KNN_TOP_MAX 16
#define SE_KNN_KS_MAX 32
int se_knn_vote(const int32_t *idx, int64_t ldi, int64_t q, int64_t list_len, const int32_t *cls, int64_t gallery,
                int num_classes, const int32_t *qidx, const int32_t *ks, int nk, int top, int32_t *out_cls,
                int32_t *out_votes, se_stream_t stream);

/*
 * Completion of given ranked lists to rankings of the whole gallery: what turns rankings that come from somewhere else (another
 * system, an approximate index, re-ranked or truncated lists) into the [q, gallery] index matrices that se_hierarchical_precision
 * and se_relevant_positions read.
 * Replaces: `ret = ret + [id for id in all_ids if id not in sret]`, class_hierarchy.py:262-264 ("IDs missing in retrieval results
 *           will be appended to the end"), the per-query Python set and list comprehension over all_ids, for a tile of queries.
 *   lists     [q, list_len] int32 gallery indices, best first (ldl elements between rows); may be NULL when list_len == 0
 *   len       [q] int32 number of valid entries of each row, in [0, list_len] (clamped to it); NULL = every row has list_len
 *   order     [gallery] int32: the all_ids order as gallery indices, a permutation of 0 .. gallery - 1; NULL = the identity
 *   rank      [q, gallery] int32 out (ldr elements between rows; elements gallery .. ldr - 1 of a row are not written)
 *   status    [q] int32 out: 0 for a clean row; bit 0: some valid entry lies outside [0, gallery); bit 1: some index occurs more
 *             than once
 * A clean row gets rank[i, :len_i] = lists[i, :len_i], followed by the elements of `order` that are not in the list, in `order`'s
 * order: exactly `gallery` entries, a permutation.  A row with status != 0 gets `order` itself (the identity when order is NULL):
 * a valid permutation, so that no consumer gathers outside its tables, but one that means nothing -- the caller looks at status
 * before it scores.  A bad row is replaced as a whole, not "keeping the first occurrence", so that the result depends neither on
 * the launch geometry nor on the order in which lanes meet a duplicate.
 * No gather leaves its row: an entry is range-checked before it is used as a bit position, nothing is read beyond len_i entries of
 * a row and nothing is written beyond `gallery` entries of a row (an element of `order` outside [0, gallery) -- a broken contract --
 * is never written).
 *   Galleries of up to SE_COMPLETE_LDS_ITEMS items keep the per-row membership bitmap in LDS (gallery / 8 bytes per workgroup)
 *   and need no workspace; larger ones keep it in se_complete_rankings_workspace_bytes(q, gallery) bytes of 4-byte aligned device
 *   scratch (one bitmap per workgroup of a capped grid), set with integer global atomics.  list_len and gallery are at most
 *   SE_COMPLETE_MAX_ITEMS.
 *   q == 0 or gallery == 0 returns SE_OK without a launch.  SE_ERR_INVALID: a NULL lists (with list_len > 0) / rank / status,
 *   ldl < list_len, ldr < gallery, a negative size or one above SE_COMPLETE_MAX_ITEMS, a workspace that is too small.
 *   Integers only: the same inputs give the same bits on every launch geometry, and nothing rests on the lane-order property that
 *   se_rank_rows_init probes.  Asynchronous on `stream`; no allocation, no host synchronisation: capturable in a HIP graph.
 */
#define SE_COMPLETE_LDS_ITEMS 262144   /* galleries up to this size keep the per-row membership bitmap in LDS */
#define SE_COMPLETE_MAX_ITEMS 1073741824
int64_t se_complete_rankings_workspace_bytes(int64_t q, int64_t gallery);
int se_complete_rankings(const int32_t *lists, int64_t ldl, const int32_t *len, int64_t q, int64_t list_len,
                         const int32_t *order, int64_t gallery, int32_t *rank, int64_t ldr, int32_t *status,
                         void *workspace, int64_t workspace_bytes, se_stream_t stream);

/*
 * Hierarchical retrieval metrics of every query from its ranking (the consumer of se_rank_rows / se_retrieve_topk).
 * Replaces: the per-query loop of ClassHierarchy.hierarchical_precision (class_hierarchy.py:211-316):
 *           P@k (WUP / LCS_HEIGHT), AHP or AHP@K (np.trapz of cum / best, :303-309), AP (:310-314), with the
 *           reference's handling of the query inside its own ranking (:280-290).
 *   rank      [q, list_len] int32 gallery indices, best first (ldr elements between rows)
 *   cls       [gallery] int32 class index of every gallery item (the kernel keeps a byte / 16-bit copy in LDS when
 *             num_classes and gallery allow);  qcls [q] class index of every query
 *   qidx      [q] int32 gallery index of the query itself (dropped from its ranking), NULL = keep everything
 *   wup, lcs  [C, C] f64 class similarity tables (Wu-Palmer, 1 - LCS height / max height)
 *   rcp       the best-possible cumulative similarity per query class (class_hierarchy.py:266,275), pre-divided
 *             for the kernel by se_hprec_reciprocal_curves (once per gallery); rcp_len = the list_len it was built
 *             for (>= this call's list_len)
 *   ks        [nk] int32 cut-offs; ahp_len: -1 no AHP, 0 whole list, K > 0 clipped AHP@K; want_ap: 0 / 1
 *   out       [q, 2 nk + 3] f64: P@k WUP x nk, P@k LCS x nk, AHP WUP, AHP LCS, AP (ldo elements between rows)
 *   order_ws  NULL, or se_hprec_order_workspace_bytes(q) bytes of 16-byte aligned device scratch: the queries are then visited in
 *             class order (one contiguous part of it per XCD), which keeps the best curve being streamed in L2.
 *             The results do not depend on it.
 */
int64_t se_hprec_order_workspace_bytes(int64_t q);
int se_hierarchical_precision(const int32_t *rank, int64_t ldr, int64_t q, int64_t list_len,
                              const int32_t *cls, int64_t gallery, const int32_t *qcls, const int32_t *qidx,
                              const double *wup, const double *lcs, int num_classes,
                              const double *rcp, int64_t rcp_len,
                              const int32_t *ks, int nk, int64_t ahp_len, int want_ap, double *out,
                              int64_t ldo, void *order_ws, se_stream_t stream);
/* The same for rankings of uint16 gallery indices (se_rank_rows with idx64 == 2; gallery <= 65,536): identical results, half the
 * ranking bytes to read.  Replaces the same lines of class_hierarchy.py:211-316. */
int se_hierarchical_precision_r16(const uint16_t *rank, int64_t ldr, int64_t q, int64_t list_len,
                                  const int32_t *cls, int64_t gallery, const int32_t *qcls, const int32_t *qidx,
                                  const double *wup, const double *lcs, int num_classes,
                                  const double *rcp, int64_t rcp_len,
                                  const int32_t *ks, int nk, int64_t ahp_len, int want_ap, double *out,
                                  int64_t ldo, void *order_ws, se_stream_t stream);

/*
 * The best-possible curves of se_hierarchical_precision, pre-divided and laid out for its loads.
 *   best_*    [num_classes, ldb] f64: for query class c, the cumulative sum of the descending-sorted similarities of
 *             the WHOLE gallery to c (class_hierarchy.py:266,275) -- host-side, once per gallery; list_len positions used
 *   rcp       [num_classes, 2, se_hprec_curve_len(list_len), 2] f64 out, per class: the divisors of the ranks BEHIND the
 *             query, (1 / (best_wup[i] - 1), 1 / (best_lcs[i] - 1)) -- dropping the query from its ranking shifts the
 *             curve and subtracts its self-similarity (class_hierarchy.py:280-290) -- then those of the ranks AHEAD of
 *             it, (1 / best_wup[i], 1 / best_lcs[i]).  Both chunk-transposed (2048-position chunks, position 8 t + e of
 *             a chunk at slot 256 e + t) so that the 256 threads of the metric kernel, each owning 8 consecutive ranks,
 *             read contiguous 16-byte pairs.
 */
int64_t se_hprec_curve_len(int64_t list_len);
int se_hprec_reciprocal_curves(const double *best_wup, const double *best_lcs, int64_t ldb,
                               int num_classes, int64_t list_len, double *rcp, se_stream_t stream);

/*
 * Normalised discounted cumulative gain of every query from its ranking, with the class similarity tables as gains: the graded,
 * position-discounted companion of se_hierarchical_precision's columns, read from the same rank tile.
 * Replaces: a host loop over pairwise_retrieval(..., return_generator=False) (the reference has no NDCG; the host statement of
 *           these semantics is ClassHierarchy.ndcg).
 *   rank, ldr, cls, qcls, qidx   exactly as in se_hierarchical_precision (qidx NULL = keep every entry)
 *   gain_a, gain_b  [C, C] f64: the gain of a retrieved item is gain[qcls[i] * C + cls[item]] (row = the query's class; no
 *             symmetry is assumed)
 *   disc      [disc_len >= list_len] f64: disc[p - 1] weighs position p (1-based, counted after the query's own entry is dropped).
 *             The kernel computes no logarithm: the caller passes 1 / log2(p + 1)
 *   ideal     [C, 2, 2, nk + 1] f64, [class][member][table][cut-off slot], slot nk = the whole list; member = 1 when
 *             qidx != NULL && qidx[i] >= 0 (the query is a gallery item: the ideal list holds one item of its class fewer)
 *   ks        [nk <= 512] int32 cut-offs >= 1, any order, duplicates allowed; a k beyond the list scores the list's end
 *   out       [q, 2 nk + 2] f64: NDCG@k of table a x nk, of table b x nk, whole-list a, whole-list b (ldo elements between rows);
 *             DCG / ideal where ideal > 0, else 0.  The last two columns are written only when want_full; without it only the
 *             first min(list_len, max(ks) + 1) ranks of a row are read (top-L lists)
 * The query's own entry is dropped where it occurs among the entries read; a member whose entry is not among them drops
 * nothing (and still takes the member = 1 ideal).  A row's result depends on that row's inputs only.  q == 0 or list_len == 0:
 * SE_OK, nothing launched.  No allocation, no host synchronisation, capturable.
 */
#define SE_NDCG_CHUNK 2048   /* ranks a workgroup takes per step (tests: list lengths around it) */
int se_ndcg(const int32_t *rank, int64_t ldr, int64_t q, int64_t list_len,
            const int32_t *cls, int64_t gallery, const int32_t *qcls, const int32_t *qidx,
            const double *gain_a, const double *gain_b, int num_classes,
            const double *disc, int64_t disc_len,
            const double *ideal,
            const int32_t *ks, int nk, int want_full,
            double *out, int64_t ldo, se_stream_t stream);

/*
 * Positions of the relevant items in every query's ranking: the exact primary data of the recall-precision curve and the mAP.
 * Replaces: the relevance list of plot_recall_precision.py:52-79 (`labels[r] == labels[qid] for r in retrieved if r != qid`).
 *   rank      [q, list_len] int32 gallery indices, best first (ldr elements between rows)
 *   cls       [gallery] int32 class index (0 .. num_classes - 1) of every gallery item; qcls [q] class index of every query
 *   qidx      [q] int32 gallery index of the query itself (dropped from its ranking), NULL = keep everything
 *   hit_off   [q + 1] int64 device array: prefix sum of R_i, the number of relevant items of query i (items of its class other
 *             than itself); built by the caller from the class counts
 *   hit_pos   [hit_off[q]] int32 out: hit_pos[hit_off[i] + j - 1] = 1-based position (query removed) of the j-th relevant item of
 *             query i.  A row stops being read once its R_i hits are found; positions of hits a row does not have read 0.
 */
int se_relevant_positions(const int32_t *rank, int64_t ldr, int64_t q, int64_t list_len,
                          const int32_t *cls, int64_t gallery, const int32_t *qcls, const int32_t *qidx,
                          int num_classes, const int64_t *hit_off, int32_t *hit_pos, se_stream_t stream);
/* The same for rankings of uint16 gallery indices (se_rank_rows with idx64 == 2; gallery <= 65,536): identical results, half the
 * ranking bytes to read.  Replaces the same lines of plot_recall_precision.py:52-79. */
int se_relevant_positions_r16(const uint16_t *rank, int64_t ldr, int64_t q, int64_t list_len,
                              const int32_t *cls, int64_t gallery, const int32_t *qcls, const int32_t *qidx,
                              int num_classes, const int64_t *hit_off, int32_t *hit_pos, se_stream_t stream);

/*
 * Average precision and recall-precision sums of a tile of queries from se_relevant_positions' output, in a fixed summation order
 * (no atomics: the same inputs give the same bits; tiles accumulate in tile order and the result does not depend on the tiling).
 * Replaces: the AP and `recprec` accumulation of plot_recall_precision.py:52-79 (average_precision_score, cumsum, max precision
 *           per recall level or per --bins bin).
 *   hit_pos, hit_off  as written / read by se_relevant_positions for these q queries
 *   order     [q] int32: the tile's queries (0 .. q - 1) sorted by class, ascending query index inside a class;
 *   class_start [num_classes + 1] int32: the queries of class c are order[class_start[c] .. class_start[c + 1])
 *   class_off [num_classes + 1] int64: prefix sum of R_c, the relevant items of every query of class c (all queries of a class
 *             must have the same R); class_len = class_off[num_classes]
 *   ap        [q] f64 out: (1 / R_i) sum_j j / p_ij, 0 when R_i = 0
 *   prec_sum  [class_len] f64 in/out: element class_off[c] + j - 1 += sum over the class's queries of j / p_j (recall level j / R_c)
 *   first_miss [num_classes] int64 in/out: += queries of the class whose first item is not relevant (recall level 0, precision 0)
 *   bins      0: no binning; B > 0 (at most 2^20): also bin_sum / bin_count [num_classes, B + 1] in/out, bin b of query i being the
 *             j with int((j / R_i) * B) == b (IEEE float64, as Python computes it): bin_sum += the max of j / p_j over the bin
 *             (0.0 for a first-position miss in bin 0), bin_count += 1, for every query of the class that has the bin
 */
int se_recall_precision_reduce(const int32_t *hit_pos, const int64_t *hit_off, int64_t q, const int32_t *order,
                               const int32_t *class_start, int num_classes, const int64_t *class_off, int64_t class_len,
                               int bins, double *ap, double *prec_sum, int64_t *first_miss, double *bin_sum,
                               int64_t *bin_count, se_stream_t stream);

/*
 * Positions of the relevant items WITHOUT a ranking: count, per relevant item, the gallery columns that precede it.
 * For a gallery that is not the query set (held-out queries against a database) no [q, n] ranking has to exist: the 1-based position
 * of a relevant item in the canonical order of se_rank_rows is the number of gallery columns in front of it, plus one.
 * Replaces: `np.argsort` + the relevance list of plot_recall_precision.py:52-79 / class_hierarchy.py:310-314 for
 *           `hierarchical_precision(retrieved, labels, ..., ignore_qids)` on a query -> gallery mapping that is not all-pairs.
 * se_count_preceding ACCUMULATES one distance slab (any tile of the gallery's columns, any shard: integer adds commute, the result
 * does not depend on tiling, launch geometry or call order) into a histogram with the layout of hit_pos:
 *   pdist     [q, n_cols] f32 distances of the q queries to gallery rows col_offset .. col_offset + n_cols (ldp elements between rows)
 *   hit_off   [q + 1] int64: query i owns cnt[hit_off[i] .. hit_off[i + 1]), one bin per relevant item (R_i of them)
 *   rel_d, rel_i [hit_off[q]] f32 / int32: distance and GLOBAL gallery index of every relevant item, per query sorted ascending in
 *             the canonical order (distance ascending, index ascending, NaN last, -0 == +0); rel_i is only ever compared
 *   qidx      [q] int32 global gallery index of the query itself (that column is skipped); NULL, or an entry < 0: not in the gallery
 *   max_rel   an upper bound of R_i the caller knows (sizes the LDS of the launch), 0 = unknown; only the speed depends on it:
 *             longer key lists, or lists above 5,460 keys, are searched in global memory
 *   cnt       [hit_off[q]] int32 in/out: for every column j other than the query's own, with p = the number of the query's relevant
 *             keys strictly before (pdist[i, j], col_offset + j):  cnt[hit_off[i] + p] += 1 if p < R_i.  A relevant column lands
 *             in its own bin; columns behind the last relevant item are not counted.  Zero it before the first slab.
 * q == 0 or n_cols == 0: SE_OK, nothing launched.  Asynchronous, no workspace, capturable.
 * se_count_to_positions: inclusive prefix sum per query, hit_pos[hit_off[i] + s] = sum of cnt[hit_off[i] + p] over p <= s -- the
 * position (query removed) of the (s + 1)-th relevant item, i.e. what se_relevant_positions writes; se_recall_precision_reduce
 * consumes it unchanged.  hit_pos may be cnt itself.
 */
int se_count_preceding(const float *pdist, int64_t ldp, int64_t q, int64_t n_cols, int64_t col_offset,
                       const int64_t *hit_off, const float *rel_d, const int32_t *rel_i, const int32_t *qidx,
                       int64_t max_rel, int32_t *cnt, se_stream_t stream);
int se_count_to_positions(const int32_t *cnt, const int64_t *hit_off, int64_t q, int32_t *hit_pos, se_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Classification side: linear SVM
 * ------------------------------------------------------------------------------------------ */

/* epilogue modes of se_svm_margin */
#define SE_SVM_GRAD 0  /* squared-hinge derivative, active-set mask, loss partial sums */
#define SE_SVM_HV 1    /* generalised Hessian-vector product's per-sample factor     */
#define SE_SVM_SCORE 2 /* decision scores                                            */

/*
 * Margins of a linear model, with a fused epilogue (fp32 MFMA; the margins themselves are never stored).
 * Replaces: the per-class X w products of scikit-learn's LinearSVC (liblinear, primal trust-region Newton solver) in
 *           LinearSVC.fit and the X coef_^T + intercept_ of decision_function (evaluate_classification_accuracy.py:43-48).
 * The objective of class column j is  f_j(w, b) = 1/2 (|w|^2 + b^2) + cpen sum_i max(0, 1 - y_ij (x_i . w + b))^2.
 *   x          [n, d] f32 samples (ldx)
 *   w          [c, d + 1] f32 (ldw >= d + 1): row j = (w_j, b_j), the bias in column d.  HV mode: the direction (v_j, v_b,j)
 *   labels     [n] int32 class of every sample; col_class [c] int32 the class of column j: y_ij = +1 if labels[i] == col_class[j],
 *              -1 otherwise (SE_SVM_GRAD only; NULL otherwise)
 *   mask       [n, ldm] uint32, ldm >= ceil(c / 32): bit j % 32 of word j / 32 of row i = active set A_ij = (1 - y_ij m_ij > 0).
 *              Written by SE_SVM_GRAD, read by SE_SVM_HV (the mask of the last gradient call), unused by SE_SVM_SCORE (NULL)
 *   out        [n, c] f32 (ldo >= c):  SE_SVM_GRAD   z_ij = -2 cpen y_ij max(0, 1 - y_ij m_ij),  m = x w^T + b
 *                                      SE_SVM_HV     z_ij = 2 cpen A_ij (x_i . v_j + v_b,j)
 *                                      SE_SVM_SCORE  s_ij = x_i . w_j + b_j
 *   loss_part  [c, ldl] f32, ldl >= se_svm_loss_blocks(n) (SE_SVM_GRAD only): element (j, r) = sum over rows 64 r .. 64 r + 63 of
 *              max(0, 1 - y_ij m_ij)^2, summed in a fixed order
 *   cpen       the penalty C of LinearSVC (> 0)
 * c >= 3 (binary problems are out of scope); every argument is checked before any device work.
 */
int64_t se_svm_loss_blocks(int64_t n);
int se_svm_margin(int mode, const float *x, int64_t ldx, int64_t n, int64_t d, const float *w, int64_t ldw,
                  int64_t c, const int32_t *labels, const int32_t *col_class, float cpen, uint32_t *mask,
                  int64_t ldm, float *out, int64_t ldo, float *loss_part, int64_t ldl, se_stream_t stream);

/*
 * Contraction over the samples: g = plus + z^T [x | 1], i.e. g[j, k] = plus[j, k] + sum_i z_ij x_ik for k < d and
 * g[j, d] = plus[j, d] + sum_i z_ij -- the gradient (plus = w) or the Hessian-vector product (plus = v) of f_j from
 * se_svm_margin's output.
 * Replaces: liblinear's X^T z products of the same solver.
 *   z [n, c] f32 (ldz), x [n, d] f32 (ldx), plus [c, d + 1] f32 (ldp) or NULL, g [c, d + 1] f32 out (ldg >= d + 1)
 *   workspace  se_svm_reduce_workspace_bytes(n, d, c) bytes, 16-byte aligned: fp32 partial tiles of fixed slices of at most 4096
 *              samples, combined per element in slice order in fp64.  No atomics: the same inputs give the same bits, and the
 *              round-off does not grow with n.
 */
int64_t se_svm_reduce_workspace_bytes(int64_t n, int64_t d, int64_t c);
int se_svm_reduce(const float *z, int64_t ldz, const float *x, int64_t ldx, int64_t n, int64_t d, int64_t c,
                  const float *plus, int64_t ldp, float *g, int64_t ldg, void *workspace,
                  int64_t workspace_bytes, se_stream_t stream);

/*
 * Per-row fp64 scalars of the solver's [c, len] f32 vectors (row j = class column j; all with leading dimension ld).
 *   se_svm_gram    out [c, nv (nv + 1) / 2] f64: sum_k v_a[j, k] v_b[j, k] for a <= b, row-major upper triangle
 *                  ((0,0), (0,1), .., (0,nv-1), (1,1), ..); 1 <= nv <= 4, unused vectors NULL
 *   se_svm_rowsum  out [c] f64: sum_k a[j, k]
 *   se_svm_axpby   out[j, k] = (float)(alpha[j] x[j, k] + beta[j] y[j, k]) evaluated in f64; alpha, beta [c] f64 device arrays;
 *                  out may alias x or y
 * Fixed reduction orders: the same inputs give the same bits.
 */
int se_svm_gram(const float *v0, const float *v1, const float *v2, const float *v3, int nv, int64_t ld, int64_t c,
                int64_t len, double *out, se_stream_t stream);
int se_svm_rowsum(const float *a, int64_t lda, int64_t c, int64_t len, double *out, se_stream_t stream);
int se_svm_axpby(const double *alpha, const float *x, int64_t ldx, const double *beta, const float *y, int64_t ldy,
                 int64_t c, int64_t len, float *out, int64_t ldo, se_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Class embeddings: similarity tables of a hierarchy, unit-sphere / spheres embeddings
 * ------------------------------------------------------------------------------------------ */

/* flags of se_class_pair_tables */
#define SE_CLASSEMB_DIAG_ONE 1 /* diagonal of the lcs table 1 (distance mode: 0), the convention of compute_class_embedding.py */
#define SE_CLASSEMB_DIST 2     /* the lcs table receives the distance h / H instead of the similarity 1 - h / H            */
#define SE_CLASSEMB_MAX_ANC 48 /* longest ancestor list of one class the pair-table kernel stages                            */

/*
 * Wu-Palmer and LCS-height tables of a list of classes.
 * Replaces: ClassHierarchy.similarity_tables (the double loop over wup_similarity / lcs) and the lcs_height loop of
 *           compute_class_embedding.py:212-216.
 * Encoding (built on the host, ClassHierarchy.pair_table_encoding): every node of the classes' ancestor closure has a preference
 * rank -- depth descending, height ascending, repr ascending, the tie-break of ClassHierarchy.lcs -- so lcs(a, b) is the common
 * ancestor of smallest rank.
 *   anc_off     [c + 1] int32 CSR offsets into anc_rank / anc_spl (nnz entries); a class's list holds itself and every ancestor,
 *               at most max_anc (1 .. SE_CLASSEMB_MAX_ANC) entries, ranks ascending
 *   anc_spl     shortest_path_length(class, ancestor) of every entry (in a DAG not always the upward distance)
 *   rank_depth, rank_height  [n_ranks] int32 depth and height of the node of every rank; max_height the hierarchy's height H >= 1
 *   wup, lcs    [c, c] f64 out (ldw / ldl elements between rows), either may be NULL (not both):
 *               wup = 2 ds / ((ds + spl_a) + (ds + spl_b)), lcs = 1 - h / H (SE_CLASSEMB_DIST: h / H), with ds / h the depth /
 *               height of lcs(a, b); IEEE divisions in float64 -- bitwise the host's values.  The diagonal of lcs is
 *               1 - h(class) / H (ClassHierarchy.similarity_tables) unless SE_CLASSEMB_DIAG_ONE
 *   missing     [1] int64 out: i c + j of the first pair (row-major, i < j) without a common ancestor, -1 if every pair has one;
 *               the tables hold NaN at such pairs (the reference raises KeyError there)
 * c = 0 is accepted (only `missing` is written).  Asynchronous; no workspace.
 */
int se_class_pair_tables(const int32_t *anc_off, const int32_t *anc_rank, const int32_t *anc_spl, int64_t nnz, int64_t c,
                         int max_anc, const int32_t *rank_depth, const int32_t *rank_height, int64_t n_ranks, int max_height,
                         int flags, double *wup, int64_t ldw, double *lcs, int64_t ldl, int64_t *missing, se_stream_t stream);

/*
 * In-place lower Cholesky factor of a symmetric float64 matrix: L L^T = A, L written over the lower triangle, exact zeros above the
 * diagonal (only the lower triangle of A is read).
 * Replaces: unitsphere_embedding (compute_class_embedding.py:14-40 -- row c solves E[:c, :c] x = S[c, :c] and sets E[c, c] =
 *           sqrt(1 - |x|^2), which is the Cholesky factor of S) and the hypersphere intersections of euclidean_embedding
 *           (:76-130), which are the Cholesky factor of the Gram matrix of the classes 1 .. n - 1 around class 0.
 *   a      [n, n] f64 (lda >= n elements between rows), in / out
 *   info   [1] int32 out (device): -1 on success, else the first row whose pivot is <= 0 or NaN (LAPACK potrf's rule, 0-based);
 *          then L[info, info] and every row after it are NaN, like the reference's sqrt of a negative; rows before it are valid
 * Blocked right-looking, block column 64, trailing update on v_mfma_f64_16x16x4_f64; no host synchronisation, no workspace;
 * n = 0 is accepted (info = -1).  Not bit-equal to LAPACK (another summation order): for a well-conditioned S with unit
 * diagonal, |L - L_lapack| and |L L^T - S| stay within a few n eps (tests/test_gpu_class_embedding.py: <= 1e-12 up to n = 8142).
 */
int se_cholesky_f64(double *a, int64_t lda, int64_t n, int32_t *info, se_stream_t stream);

/* info codes of se_eigh_f64 below zero (>= 0: converged, the number of sweeps used) */
#define SE_EIGH_NOT_CONVERGED (-1) /* off(A) still above the tolerance after max_sweeps sweeps; w / v hold the state reached    */
#define SE_EIGH_NONFINITE (-2)     /* the input holds a NaN or an infinity (or |A|_F^2 overflows); w / v are NaN                */

/*
 * Eigendecomposition of a symmetric float64 matrix: A = V diag(w) V^T, eigenvalues ascending, eigenvectors the COLUMNS of V in the
 * same order (the conventions of numpy.linalg.eigh).
 * Replaces: the np.linalg.eigh of sim_approx (compute_class_embedding.py:44-72, the eigenvectors of the class similarities scaled
 *           by the roots of their eigenvalues) and of mds (:134-160, classical multidimensional scaling of the class distances).
 *   a          [n, n] f64 (lda >= n elements between rows), in; DESTROYED (on return its diagonal holds the unsorted eigenvalues).
 *              Taken as symmetric: both triangles are read
 *   w          [n] f64 out, ascending
 *   v          [n, n] f64 out (ldv >= n elements between rows); v[:, j] belongs to w[j]; elements past column n are not touched
 *   workspace  se_eigh_f64_workspace_bytes(n) bytes of device memory, 8-byte aligned (n^2 doubles for the unsorted eigenvectors,
 *              one 64 x 64 rotation per block pair, the reduction scratch); -1 from the size query: n is out of range
 *   info       [1] int32 out (device): the number of sweeps used (0 for a matrix that is diagonal already), or SE_EIGH_NOT_CONVERGED
 *              (w / v finite: the diagonal and the rotations reached so far), or SE_EIGH_NONFINITE (w / v all NaN, no sweep run)
 *   max_sweeps >= 0, the bound of the outer loop (random matrices take 5 to 8 sweeps, the clustered class spectra up to 28)
 * Two-sided block Jacobi, blocks of 32 columns, round-robin ordering (se_eigh_schedule over nb = 2 ceil(n / 64) blocks, the matrix
 * padded with zeros that are never stored): per round one workgroup per block pair diagonalises its 64 x 64 sub-block by cyclic
 * Jacobi in LDS (bounded inner sweeps; a rotation whose entry is exactly 0 is skipped, so the padding never mixes with real rows),
 * then A[:, pair] J, V[:, pair] J and J^T A[pair, :] run on v_mfma_f64_16x16x4_f64.  The host reads off(A)^2 = sum_{i != j} a_ij^2
 * once per sweep and stops at off(A) <= sqrt(n) 2^-53 |A|_F: the call SYNCHRONISES the stream (once per sweep and at the end).
 * Signs, and the basis inside a cluster of equal eigenvalues, are unspecified.  Not bit-equal to LAPACK; eigenvalues, residual
 * A V - V diag(w) and V^T V - I stay within a few n eps (tests/test_gpu_eigh.py).  n = 0 is accepted (info = 0, nothing else
 * written); n > 131072 is SE_ERR_UNSUPPORTED.
 */
int64_t se_eigh_f64_workspace_bytes(int64_t n);
int se_eigh_f64(double *a, int64_t lda, int64_t n, double *w, double *v, int64_t ldv, void *workspace, int32_t *info, int max_sweeps,
                se_stream_t stream);

/*
 * The rounds of one sweep of se_eigh_f64 over nb blocks (nb even, >= 2), by the circle method: pairs [nb - 1, nb / 2, 2] int32
 * HOST memory out, pairs[r, k] = (lo, hi) with lo < hi.  Within a round the pairs are disjoint; over the nb - 1 rounds every
 * unordered pair of blocks occurs exactly once.  Round r pairs block r with block nb - 1 and, for k = 1 .. nb / 2 - 1, block
 * (r + k) mod (nb - 1) with block (r - k) mod (nb - 1).  Host only (no device work; sehip.eigh_schedule states the same rule).
 */
int se_eigh_schedule(int nb, int32_t *pairs);

/* ------------------------------------------------------------------------------------------
 * Input pipeline: batches of file-based datasets composed on the device
 * ------------------------------------------------------------------------------------------ */

/*
 * One launch composes a batch [B, ch, cw, 3] (NHWC) from variable-sized uint8 RGB images resident in device memory.
 * Replaces: datasets/common.py:380-581 (FileDatasetGenerator.compose_batch, _load_image, _transform: Pillow's bilinear resize of
 *           the decoded image, float conversion, normalisation, optional BGR order, random flip, random erasing, random / centre
 *           crop with reflect padding).  The kernel knows nothing of crop, pad or flip: the host folds them into the tables
 *           (sehip.resample_tables), which are indexed by OUTPUT coordinate.
 *   arena    uint8 store of arena_bytes bytes; image b starts at src_off[b], rows packed (src_w * 3 bytes), RGB interleaved
 *   src_off  [B] int64;  src_hw [B, 2] int32 = (h, w)
 *   xmap     [B, cw, 3] int32 = (u, xmin, n): u the coordinate of that output column in the zoomed, already flipped image (used
 *            by the erase test only), xmin the first source column, n the number of taps;  xk [B, cw, Kx] int32: Pillow's 22-bit
 *            fixed-point weights, zero-padded to Kx
 *   ymap     [B, ch, 3], yk [B, ch, Ky]: the same for rows
 *   erase    [B, 4] int32 = (y, x, h, w) in zoomed, flipped coordinates; h == 0: none
 *   seed     [B] uint32 noise seed of the erase rectangle
 *   mean, std  [3] f32 (device) in RGB order;  bgr != 0: source channel c is written at position 2 - c
 *   out      [B, ch, cw, 3] f32 (SE_DTYPE_F32) or bf16 (SE_DTYPE_BF16: the f32 value rounded to nearest even)
 * For output (b, cy, cx) and source channel c:
 *     t(r) = clip8((2^21 + sum_i xk[cx, i] * src[r, xmin_x + i, c]) >> 22)        horizontal pass, uint8 result
 *     v    = clip8((2^21 + sum_j yk[cy, j] * t(ymin_y + j)) >> 22)                vertical pass
 *     out  = (float(v) - mean[c]) / std[c]                                        IEEE f32 subtract and divide
 * -- Pillow's 8-bit resampling, bit for bit; an axis whose size does not change takes the single tap 1 << 22.  Where u_y is in
 * [y, y + h) and u_x in [x, x + w) the value is (U - mean[c']) / std[c'] instead, c' the channel's POSITION in the output (the
 * reference normalises its noise with the RGB-ordered statistics by position, common.py:538-540) and U uniform in [0, 255) from a
 * counter-based hash of (seed[b], u_y, u_x, c'): the same arguments give the same noise.
 * Table entries are clamped to the image (0 <= xmin < w, n <= min(Kx, w - xmin), likewise rows), and a sample whose image does not
 * lie inside the arena is written as NaN.  SE_ERR_UNSUPPORTED when one output row's taps (Ky rows of cw pixels) and the column
 * table (cw x Kx weights) exceed the 64 KB of LDS a workgroup owns, or B > 65535.  Asynchronous; no workspace; B = 0 is accepted.
 */
int se_image_batch(const void *arena, int64_t arena_bytes, const int64_t *src_off, const int32_t *src_hw, const int32_t *xmap,
                   const int32_t *xk, const int32_t *ymap, const int32_t *yk, const int32_t *erase, const uint32_t *seed,
                   const float *mean, const float *std, int bgr, void *out, int out_dtype, int64_t B, int ch, int cw, int Kx, int Ky,
                   se_stream_t stream);

/*
 * One launch composes a batch [B, H, W, C] (NHWC) from a store of small float32 images resident in device memory: gather, Keras'
 * affine random_transform with bilinear interpolation, both flips, standardisation, layout and dtype conversion.
 * Replaces: datasets/common.py:638-670, 771-796 (TinyDatasetGenerator: ImageDataGenerator.random_transform + standardize per sample
 *           [third party: keras_preprocessing 1.0.x], i.e. scipy.ndimage.affine_transform(order = 1) channel by channel, the flips,
 *           then (x - mean) / (std + 1e-6)).
 *   images   [N, H, W, C] f32, raw un-normalised pixels; C in 1 .. 4, H, W >= 1
 *   index    [B] int64: the store row of every sample, any order, repeats allowed; a value outside [0, N) writes that sample as NaN
 *   affine   [B, 6] FLOAT64 = (M00, M01, M02, M10, M11, M12): output (row, col) -> source (row, col)
 *   flags    [B] int32: bit 0 horizontal flip, bit 1 vertical flip (applied AFTER the transform, as Keras does)
 *   mean, stdp  [C] f32; stdp already holds std + 1e-6
 *   fill_mode  SE_FILL_NEAREST / SE_FILL_CONSTANT / SE_FILL_REFLECT;  cval: the value of 'constant' outside the image
 *   out      [B, H, W, C] f32 (SE_DTYPE_F32) or bf16 (SE_DTYPE_BF16: the f32 value rounded to nearest even)
 * For output (b, r, c) and channel k, in float64 with every operation separately rounded, in the order of scipy's NI_GeometricTransform:
 *     r' = vflip ? H - 1 - r : r,   c' = hflip ? W - 1 - c : c
 *     y  = (r' * M00 + c' * M01) + M02,   x = (r' * M10 + c' * M11) + M12
 * Per axis of length n with coordinate v:
 *     nearest   v stays; taps i0 = floor(v) and i0 + 1, each clamped to [0, n - 1] (outside the image both are the edge pixel)
 *     constant  v < 0 or v > n - 1 on ANY axis: the pixel is cval (no interpolation beyond the edges); otherwise as nearest
 *     reflect   n == 1: v = 0.  v < 0: p = 2 n; if v < -p: v = p * trunc(-v / p) + v; then v = (v < -n) ? v + p : -v - 1.
 *               v > n - 1: v = v - p * trunc(v / p); if v >= n: v = p - v - 1.  Taps i0 = floor(v) (may be -1) and i0 + 1, each
 *               folded: m = mod(i, 2 n); idx = m < n ? m : 2 n - 1 - m
 * With f = v - floor(v), the weights w0 = 1 - f and w1 = 1 - w0 of each axis and the four taps a00 .. a11 (first digit: row):
 *     t   = (((0 + (a00 * wy0) * wx0) + (a01 * wy0) * wx1) + (a10 * wy1) * wx0) + (a11 * wy1) * wx1
 *     out = (float(t) - mean[k]) / stdp[k]                    float(): round to nearest even; IEEE f32 subtract and divide
 * and float(cval) in the place of float(t) for a 'constant' pixel outside (Keras standardises after the transform) -- bit for bit what
 * scipy.ndimage.affine_transform(x, M[:2, :2], M[:2, 2], order = 1, mode, cval) into a float32 array, the flips and the float32
 * standardisation give (tests/golden/tiny_affine.npz).
 * Every tap is inside its image whatever the matrix holds.  One output element per thread and trip, no LDS, no atomics: the same
 * bits whatever the launch geometry.  int64 element offsets; the grid is capped at SE_TINY_BATCH_MAX_BLOCKS workgroups of 256
 * threads that stride over the batch.  B = 0 returns SE_OK without a launch; a negative B or N, H or W < 1, C outside 1 .. 4, an
 * unknown fill mode or output dtype, or a NULL pointer with B > 0 is SE_ERR_INVALID; H * W * C > 2^30 is SE_ERR_UNSUPPORTED.
 * Asynchronous; no workspace; capturable in a HIP graph.
 */
#define SE_FILL_NEAREST 0
#define SE_FILL_CONSTANT 1
#define SE_FILL_REFLECT 2
#define SE_TINY_BATCH_MAX_BLOCKS 2048
int se_tiny_batch(const float *images, int64_t N, const int64_t *index, const double *affine, const int32_t *flags, const float *mean,
                  const float *stdp, int fill_mode, float cval, void *out, int out_dtype, int64_t B, int H, int W, int C,
                  se_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bootstrap over queries: confidence intervals and paired tests of the retrieval metrics
 * ------------------------------------------------------------------------------------------ */

/*
 * Means of per-query metric rows resampled with replacement, one launch for all replicates.
 * Replaces: the host composition idx = randint(q, size = (R, q)); vals[idx].mean(axis = 1) (the reference prints bare means; the
 *           evaluation tools resample se_hierarchical_precision's per-query rows, bootstrap.py).
 *   vals   [q, m] float64, row pitch ldv >= m;  1 <= q <= 2^31 - 1,  1 <= m <= SE_BOOTSTRAP_COLS_MAX
 *   seed   64 bits, read as UNSIGNED (int64_t only carries them)
 *   out    [reps, m] float64, row pitch ldo >= m:  for rep0 <= r < rep0 + reps and c < m
 *              out[r - rep0, c] = S / (double)q,   S = the float64 sum over t = 0 .. q - 1 of vals[idx(seed, r, t, q), c]
 *          (columns m .. ldo - 1 of out stay as they are; columns m .. ldv - 1 of vals are never read)
 *
 * THE INDEX STREAM idx(seed, r, t, q) IS PART OF THIS ABI: the same seed gives the same replicates on every machine and in every
 * later version, and two tables of the same q resampled with one seed are resampled with the same queries (paired).
 *   Draw t of replicate r uses block b = t >> 1 and half h = t & 1.
 *   (x0, x1, x2, x3) = Philox4x32-10(counter, key):
 *       counter = (b & 0xffffffff, b >> 32, r & 0xffffffff, r >> 32)
 *       key     = (seed & 0xffffffff, seed >> 32)
 *   Multipliers are M0 = 0xD2511F53 on counter word 0 and M1 = 0xCD9E8D57 on counter word 2.
 *   Key increments per round are 0x9E3779B9 (k0) and 0xBB67AE85 (k1), added after each of the first nine rounds.
 *   Each of the ten rounds computes: c <- (hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0)).
 *   u = x[2h] | x[2h + 1] << 32, and idx = (u * q) >> 64, the high half of the 128-bit product.  The bias is q / 2^64.
 * 0 <= idx < q for every u, so every gather is inside the table whatever the seed.
 * Known answers: Philox(counter 0,0,0,0; key 0,0) = 6627e8d5 e169c58d bc57ac4c 9b00dbd8;  seed 0, r 0, q 10, t 0..7: 8 6 3 0 3 2 4 4.
 *
 * SUMMATION ORDER (float64, no floating-point atomics; fixed by q and m alone, never by reps, rep0 or the launch geometry):
 *   there are 256 chains; chain j starts at +0 and adds, in ascending t, the draws of the blocks b = j, j + 256, j + 512, ...
 *   (draw 2 b, then draw 2 b + 1 where that is < q);
 *   the chains of each group of 64 (j >> 6) combine in a butterfly: for off = 32, 16, 8, 4, 2, 1: s[l] <- s[l] + s[l ^ off];
 *   the four group sums w0 .. w3 are added as ((w0 + w1) + w2) + w3, and that sum is divided by (double)q.
 * The same inputs give the same bits, and a call for replicates 0 .. 9 equals the calls for 0 .. 3 and 4 .. 9 put together.  A NaN in
 * a drawn row makes that replicate's column NaN (and no other).
 * reps == 0 returns SE_OK without a launch.  q or m out of range, ldv < m, ldo < m, rep0 < 0, reps < 0, or a NULL pointer with
 * reps > 0 is SE_ERR_INVALID.  Asynchronous on `stream`; no workspace, no allocation, no host synchronisation; capturable in a HIP
 * graph.  A row is read by one lane: rows that do not cross a 128-byte line (an aligned base and a power-of-two pitch of >= m
 * doubles, which sehip.bootstrap_means makes) cost one line per draw.
 */
#define SE_BOOTSTRAP_COLS_MAX 16
int se_bootstrap_means(const double *vals, int64_t ldv, int64_t q, int m, int64_t seed, int64_t rep0, int64_t reps, double *out, int64_t ldo,
                       se_stream_t stream);

/*
 * The index stream of se_bootstrap_means on its own (the same device function):
 *     out[r - rep0, t - t0] = idx(seed, r, t, q)     for rep0 <= r < rep0 + reps and t0 <= t < t0 + count <= q
 *   out  [reps, count] int32, row pitch ldo >= count.  1 <= q <= 2^31 - 1: with a small window the stream can be read at sizes at
 *        which no value table would fit.
 * reps == 0 or count == 0 returns SE_OK without a launch.  q out of range, a window outside [0, q], ldo < count, rep0 < 0, reps < 0, or
 * a NULL out with work to do is SE_ERR_INVALID.  Asynchronous; no workspace; capturable in a HIP graph.
 */
int se_bootstrap_indices(int64_t q, int64_t seed, int64_t rep0, int64_t reps, int64_t t0, int64_t count, int32_t *out, int64_t ldo,
                         se_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEHIP_H */
