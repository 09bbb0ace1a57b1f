/*
 * bayeslm.h -- C ABI of libbayeslm_hip.so (MI355X / gfx950 only).
 *
 * The reference (AmourWaltz/BayesLMs) has no FFI of its own: its hot path is
 * Python calling ATen/cuDNN ops.  Each entry point below
 * replaces the device work of one group of those call sites; the citation on
 * each declaration is the reference line(s) it stands in for
 * (paths relative to steps/pytorchnn/).
 *
 * Contract:
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory
 *     owned by the caller (PyTorch's caching allocator in the Python host);
 *   - the library allocates nothing persistent and keeps no references;
 *   - every call is asynchronous on the hipStream_t passed in (void* here so
 *     the header needs no HIP include); no internal synchronisation;
 *   - returns 0 (BLM_OK) or a negative blm_status; blm_last_error() gives a
 *     thread-local message; nothing throws or aborts;
 *   - all tensors fp32 row-major unless stated; token ids int64.
 */
#ifndef BAYESLM_H
#define BAYESLM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLM_ABI_VERSION 1u

typedef enum blm_status {
  BLM_OK = 0,
  BLM_ERR_INVALID = -1,   /* bad shape / null pointer / misaligned operand   */
  BLM_ERR_ABI = -2,       /* abi_version mismatch                            */
  BLM_ERR_HIP = -3,       /* a HIP runtime call failed (message has detail)  */
  BLM_ERR_UNSUPPORTED = -4
} blm_status;

/* Philox4x32-10 stream ids: counter = (block_lo, block_hi, stream, step),
 * key = seed.  Must match oracle/philox.py. */
#define BLM_STREAM_WEIGHT  0x10000000u  /* class in the top 4 bits + tensor id (low 28 bits) */
#define BLM_STREAM_DROPOUT 0x20000000u  /* + site id */
#define BLM_STREAM_LRT     0x30000000u  /* + site id: the pre-activation noise of local reparameterisation */
#define BLM_STREAM_SWAG    0x40000000u  /* + 0: a SWAG sample's diagonal noise, + 1: its low-rank noise; step = sample id */
#define BLM_STREAM_LAPLACE 0x50000000u  /* the logit noise of the last-layer Laplace predictive; step = sample id */
#define BLM_STREAM_SGMCMC  0x60000000u  /* the Langevin noise of an SG-MCMC weight update; step = optimisation step */

typedef struct blm_rng {
  uint64_t seed;    /* Philox key                                             */
  uint32_t stream;  /* BLM_STREAM_* + id                                      */
  uint32_t step;    /* optimisation step: same (seed,stream,step) => same eps */
} blm_rng;

/* --------------------------------------------------------------------------
 * Library info
 * ------------------------------------------------------------------------ */
uint32_t    blm_abi_version(void);
const char* blm_last_error(void);
/* Fills gfx arch name (<= 31 chars), CU count and LDS bytes/CU of device
 * `device`; used by the host to refuse anything that is not gfx950. */
int blm_query(int device, char* arch32, int* n_cu, int* lds_bytes);

/* --------------------------------------------------------------------------
 * Variational weights: W = mu + exp(lgstd) * eps, and the KL term
 * ------------------------------------------------------------------------ */

/* Describes the variational part of a weight matrix W (rows x cols, leading
 * dimension ld): rows [row_lo, row_lo + srows) carry noise, lgstd is
 * (srows x cols) with leading dimension cols.
 *   BayesLinear: row_lo = 0, srows = rows        (model.py:1083-1107)
 *   Bayes2LSTM : row_lo = (pos-1)*H, srows = H   (model.py:716-725)
 * eps != NULL  -> injected noise (srows x cols), used for parity tests;
 * eps == NULL  -> Philox noise from `rng`, element index = r*cols + c with
 *                 r relative to row_lo.
 * lgstd == NULL -> no noise at all (eval mode / mean weights). */
typedef struct blm_variational {
  const float* lgstd;
  const float* eps;
  int32_t row_lo;
  int32_t srows;
  blm_rng rng;
} blm_variational;

/* Materialise W (rows x cols, contiguous) from mu in one pass and, if
 * kl_out != NULL, add  kl_weight * mean(mu_s^2 - 2 lgstd + exp(2 lgstd))/2
 * (mu_s = the noisy rows of mu) to *kl_out.
 * Replaces model.py:1083-1107 (BayesLinear.sample_weight_diff/_flat_weights),
 * :668-732 (Bayes2LSTM.sample_weight_diff/flat_parameters), :1243-1249.
 * Bias vectors: pass rows = len, cols = 1. */
int blm_sample_weight(const float* mu, int64_t rows, int64_t cols, const blm_variational* v,
                      float* w_out, float* kl_out, float kl_weight, void* stream);

/* Backward of blm_sample_weight: dmu[r,c] += dW[r,c] for all rows;
 * dlgstd[r',c] += dW[row_lo+r',c] * eps * exp(lgstd) on the noisy rows (eps
 * injected or regenerated from the counter).  SURVEY.md Appendix C. */
int blm_sample_weight_bwd(const float* dw, int64_t rows, int64_t cols, const blm_variational* v,
                          float* dmu, float* dlgstd, void* stream);

/* Write the N(0,1) stream itself (n floats): test/debug visibility of the
 * generator the fused paths use. */
int blm_philox_normal(float* out, int64_t n, const blm_rng* rng, void* stream);

/* *out += weight * mean(mu^2 - 2 lg + exp(2 lg) [- 1]) / 2 over an
 * (rows x cols) window; mu has leading dimension ld_mu, lg is contiguous.
 * Replaces model.py:1109-1125, :734-765, :1251-1256, :1816-1826. */
int blm_kl_mean_fwd(const float* mu, int64_t ld_mu, const float* lgstd, int64_t rows, int64_t cols,
                    int minus_one, float weight, float* out, void* stream);
/* dmu += g * mu / n ; dlg += g * (exp(2 lg) - 1) / n   (n = rows*cols; g is
 * the upstream scalar gradient times the same weight, read from device).
 * SURVEY.md Appendix C. */
int blm_kl_mean_bwd(const float* mu, int64_t ld_mu, const float* lgstd, int64_t rows, int64_t cols,
                    const float* g_dev, float weight, float* dmu, int64_t ld_dmu, float* dlgstd, void* stream);

/* All variational tensors of a module in ONE launch per direction (Bayes2LSTM samples 8 tensors and takes the KL
 * of 4 of them every step, model.py:668-732 + :734-765: 8 + 4 + 4 + 8 launches of the single-tensor entry points).
 * Item i:  W_i = mu_i (+ exp(lgstd_i) * eps on the rows [row_lo, row_lo + srows))      -> w_out (NULL: KL only)
 *          *kl_out += kl_weight_i * sum(mu_s^2 - 2 lgstd + exp(2 lgstd) - kl_minus_i) / (2 * srows * cols)
 *                     (kl_weight 0: no KL from this item; kl_weight = n / count re-bases the mean, model.py:737-740).
 * blm_variational_group_fwd sets *kl_out = 0 first (kl_out may be NULL when no item has a KL weight).
 * Backward, g = *kl_grad (device scalar, NULL = no KL gradient), n = srows * cols:
 *          dmu_i    += dw_i                          (all rows; dw NULL: skipped)
 *          dmu_i    += g * kl_weight_i * mu / n      (noisy rows)
 *          dlgstd_i += dw_i * eps * exp(lgstd) + g * kl_weight_i * (exp(2 lgstd) - 1) / n
 * = blm_sample_weight_bwd + blm_kl_mean_bwd of every item.  At most BLM_VAR_GROUP_MAX items. */
#define BLM_VAR_GROUP_MAX 16
typedef struct blm_var_item {
  const float* mu;
  int64_t rows, cols;
  blm_variational v;
  float* w_out;
  float kl_weight;
  float kl_minus;
  const float* dw;
  float* dmu;
  float* dlgstd;
} blm_var_item;
int blm_variational_group_fwd(const blm_var_item* items, int32_t n, float* kl_out, void* stream);
int blm_variational_group_bwd(const blm_var_item* items, int32_t n, const float* kl_grad, void* stream);

/* --------------------------------------------------------------------------
 * Local reparameterisation (opt-in; csrc/lrt.hip).  No reference counterpart: the reference has the one-shared-W estimator
 * above only.  For a BayesLinear weight (mu, lgstd: N x K) and input rows x (M x K) the layer's PRE-ACTIVATIONS are sampled,
 *   m = x mu^T,   v = x^2 (sigma^2)^T,   s = sqrt(v),   y = m + s * zeta,    sigma^2 = exp(2 lgstd),
 * zeta ~ N(0,1) independent per (row, column); backward, given dy, with q = dy * zeta / (2 s) and q = 0 where s == 0:
 *   dmu = dy^T x,   dlgstd = 2 sigma^2 * (q^T x^2),   dx = dy mu + 2 x * (q sigma^2)          (* elementwise)
 * The six products are blm_gemm calls of the caller (bayeslms_amd/ops.py: bayes_linear_lrt); the entry points below are the
 * elementwise passes between them.  None of them reduces anything: results are bit-identical run to run in every mode.
 *
 * zeta: an (M, N) tensor handed in (parity tests), or, zeta == NULL, Philox noise from `rng` (stream BLM_STREAM_LRT + site id)
 * generated in registers and never stored: y is seen as a (rows, B, N) activation, M = rows * B, and element (row, b, n) takes
 * value ((row * global_cols + col_offset + b) * N + n) of the stream, as the dropout masks are keyed (global_cols 0 = B), so a
 * data-parallel rank draws the columns of the one-process run and backward regenerates what forward drew.
 * 16-byte accesses when N % 4 == 0 and the operands are 16-byte aligned, a guarded scalar loop otherwise.
 * ------------------------------------------------------------------------ */
/* dst[i] = src[i]^2 (mode 0: x^2) or exp(2 src[i]) (mode 1: sigma^2 from lgstd), i < n. */
int blm_lrt_prepare(const float* src, float* dst, int64_t n, int mode, void* stream);
/* In place: y holds m and receives y = m + sqrt(v) * zeta; s holds v and receives s = sqrt(v), which backward needs. */
int blm_lrt_combine(float* y, float* s, const float* zeta, const blm_rng* rng, int rows, int B, int N, int col_offset,
                    int global_cols, void* stream);
/* q = dy * zeta / (2 s), 0 where s == 0; zeta handed in or regenerated exactly as blm_lrt_combine took it. */
int blm_lrt_bwd_factor(const float* dy, const float* s, float* q, const float* zeta, const blm_rng* rng, int rows, int B, int N,
                       int col_offset, int global_cols, void* stream);
/* out[i] = (accumulate ? out[i] : 0) + scale * a[i] * b[i], i < n; out may be a or b.  dlgstd += 2 sigma^2 * (q^T x^2) and
 * 2 x * (q sigma^2) of the formulas above. */
int blm_lrt_mul(float* out, const float* a, const float* b, int64_t n, float scale, int accumulate, void* stream);

/* --------------------------------------------------------------------------
 * fp32 MFMA GEMM family (v_mfma_f32_32x32x2_f32, LDS tiled)
 * ------------------------------------------------------------------------ */
typedef enum blm_gemm_op {
  BLM_GEMM_NT = 0, /* C[M,N] = A[M,K] * B[N,K]^T   forward  F.linear      */
  BLM_GEMM_NN = 1, /* C[M,N] = A[M,K] * B[K,N]     dgrad    dX = dY W     */
  BLM_GEMM_TN = 2  /* C[M,N] = A[K,M]^T * B[K,N]   wgrad    dW = dY^T X   */
} blm_gemm_op;

typedef enum blm_epilogue {
  BLM_EPI_NONE = 0,
  BLM_EPI_BIAS = 1,        /* C = acc + bias[n]                                        */
  BLM_EPI_BIAS_GELU = 2,   /* z = acc + bias[n]; C = gelu_erf(z)*keep; aux[m,n] = gelu_erf'(z)*keep (if aux) */
  BLM_EPI_MUL_DGELU = 3,   /* C = acc * aux[m,n]   (aux as written by BIAS_GELU: GELU' and dropout in one factor) */
  BLM_EPI_BAYES_WGRAD = 4, /* TN only, C = dmu, C2 = dlgstd, see below                 */
  BLM_EPI_GP_MIX = 5,      /* z = acc + bias; aux = z; C = sum_i act_i(z) coef[i,n]     */
  BLM_EPI_MUL_DGP_MIX = 6, /* C = acc * sum_i act_i'(aux) coef[i,n]; C2 (optional) = acc (after dropout) */
  BLM_EPI_CE_PART = 7,     /* internal to blm_linear_nll (blm_gemm refuses it): no C, per-tile softmax partials instead */
  BLM_EPI_MC_PART = 8,     /* internal to blm_linear_mc_stats (blm_gemm refuses it): no C, per-tile uncertainty partials */
  BLM_EPI_MC_LOGP = 9      /* internal to blm_linear_mc_logprobs (blm_gemm refuses it): MC_PART, and C = log pbar per token */
} blm_epilogue;

#define BLM_GEMM_ACCUMULATE 1u /* C (+= C2) accumulate into existing contents */

typedef struct blm_gemm_args {
  uint32_t abi_version; /* BLM_ABI_VERSION */
  int32_t op;           /* blm_gemm_op */
  int32_t M, N, K;
  const float* A; int64_t lda;
  const float* B; int64_t ldb;
  float* C;       int64_t ldc;
  float alpha;          /* C = alpha * acc (+ epilogue)                        */
  uint32_t flags;       /* BLM_GEMM_ACCUMULATE                                 */
  int32_t epilogue;     /* blm_epilogue */
  const float* bias;    /* [N]                                                 */
  float* aux;           /* [M,N] ld = ldc: pre-activation (written or read)    */
  const float* coef;    /* GP mixture coefficients [4,N]: tanh,sigmoid,relu,gelu */
  /* Variational B operand (NT, NN): B is the *mean* matrix mu and the tile
   * loader forms W = mu + exp(lgstd)*eps on the fly (fused sampling, no W in
   * HBM).  var_b.lgstd == NULL -> B used as is.
   * model.py:1127-1129 fwd; autograd dX of the same. */
  blm_variational var_b;
  /* BLM_EPI_BAYES_WGRAD (TN; C has the shape of W):
   *   dW  = alpha*acc
   *   C [n,k] (+)= dW + kl_lambda * mu/n_kl      (KL part on noisy rows only)
   *   C2[r,k] (+)= dW*eps*exp(lgstd) + kl_lambda*(exp(2 lgstd)-1)/n_kl
   *               for rows r = n - row_lo in [0, srows)
   * with mu = wg_mu (ld = ldc), var_c describing lgstd/eps/rng, and
   * 1/n_kl = kl_inv_n (the element count of the mean the KL term belongs to:
   * srows*N for BayesLinear, H*(H+E) for a Bayes2LSTM matrix, model.py:737-740).
   * The KL part only touches the noisy rows of mu.
   * (autograd of model.py:1083-1107 + :1109-1125). */
  float* C2;
  const float* wg_mu;
  blm_variational var_c;
  float kl_lambda;
  float kl_inv_n;
  /* Dropout fused into the activation epilogues (drop_p > 0): C is seen as a
   * (rows, drop_B, N) activation, m = row*drop_B + b, mask keyed by the global
   * element (row, drop_col_offset + b, n) of a tensor with drop_global_cols
   * columns.  BIAS_GELU / GP_MIX: C = act(z) * keep/(1-p) (BIAS_GELU also folds keep
   * into aux);  MUL_DGP_MIX: C = acc * keep/(1-p) * act'(aux).  (model.py:1043 dropout) */
  float drop_p;
  blm_rng drop_rng;
  int32_t drop_B, drop_col_offset, drop_global_cols;
  /* TN only (wgrad dW = dY^T X, A = dY): colsum_a[m] += alpha * sum_k A[k,m], i.e. the bias
   * gradient of the same layer, taken from the A tiles the kernel stages anyway. */
  float* colsum_a;
} blm_gemm_args;

int blm_gemm(const blm_gemm_args* a, void* stream);

/* Arithmetic of the GEMM family's matrix instruction (process-wide; default BLM_GEMM_MODE_F32, or the
 * BLM_GEMM_MODE=bf16x3 environment variable at first use).
 *   F32:    v_mfma_f32_32x32x2_f32 on the fp32 operands -- the parity mode, what every reported number uses.
 *   BF16X3: OPT-IN.  Each fp32 operand value is split into bf16 hi + lo when a wave reads its fragment and
 *           A.B is formed as hi.hi + hi.lo + lo.hi on v_mfma_f32_32x32x16_bf16 (fp32 accumulate): same
 *           memory traffic, 5.3x less matrix-pipe time, 4.5e-6 max relative error at K = 4096 against
 *           3.6e-7.  Lower precision than the reference's fp32: never on by default.  Applies to the
 *           aligned fast path (LDS-DMA loaders) without fused sampling; other launches stay F32.
 *   BF16X6: OPT-IN.  Three parts (hi + mid + lo = the full 24-bit mantissa, an exact representation) and the six
 *           largest part products: an fp32-accurate multiply, 2.7x less matrix-pipe time than F32. */
#define BLM_GEMM_MODE_F32 0
#define BLM_GEMM_MODE_BF16X3 1
#define BLM_GEMM_MODE_BF16X6 2
int blm_set_gemm_mode(int mode);
int blm_get_gemm_mode(void);

/* Inference only: nll[m] = logsumexp_n(x[m,:] . w[n,:] + bias[n]) - (x[m,:] . w[tgt[m],:] + bias[tgt[m]]) without storing the
 * M x N logits -- the decoder product's epilogue keeps one (max, sum of exp) pair per row and column tile, a second small
 * kernel folds them (csrc/gemm_api.hip).  Replaces decoder + log_softmax + gather of train.py:452-455 (evaluate) and
 * compute_sentence_scores_bayes_jianwei.py:157-170 (one model; two models: blm_linear_nll2 below).  bias may be NULL; lse
 * (optional) receives the log-sum-exp per row; a target outside [0, N) gives NaN for its row;
 * ws: blm_linear_nll_ws_floats(M, N) floats, 16-byte aligned, owned by the caller.  N % 4 == 0. */
int64_t blm_linear_nll_ws_floats(int M, int N);
int blm_linear_nll(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const int64_t* tgt,
                   float* nll, float* lse, float* ws, int M, int N, int K, void* stream);
/* Token-level predictive uncertainty from S Monte-Carlo weight samples, inference only; no reference counterpart (the
 * reference scores with mean weights).  For token m and sample s < S the logits are z[s,v] = x[m,s].w[v] + b[v], v < V:
 *   lse_s = logsumexp_v z[s,v],   p[s,v] = exp(z[s,v] - lse_s),   pbar[v] = (1/S) sum_s p[s,v]
 *   nll_s[m,s] = lse_s - z[s,tgt[m]]                        (optional; what blm_linear_nll gives for that row)
 *   bma_nll[m] = -log pbar[tgt[m]] = -log((1/S) sum_s exp(-nll_s[m,s]))   (computed with a max shift)
 *   h_pred[m]  = -sum_v pbar[v] log pbar[v]                 (0 log 0 = 0: predictive entropy of the model average)
 *   mi[m]      = (1/S) sum_s sum_v p[s,v] (log p[s,v] - log pbar[v])   (mean_s KL(p_s || pbar): the epistemic part)
 * mi is computed in this KL form, never as h_pred - mean_s H[p_s] (two ~10-nat entropies whose fp32 difference loses small
 * values): mi >= 0 up to rounding, and the expected entropy is h_pred - mi.  A target outside [0, V) gives NaN for that token's
 * nll_s and bma_nll.
 * Layout: x is token-major, Sp = S rounded up to a power of two, 1 <= S <= 64: row m * Sp + s holds sample s of token m; rows
 * with s >= S are padding and enter no statistic.  w and bias have Np = V rounded up to 4 rows, 16-byte aligned; columns >= V
 * enter no statistic (masked, whatever w / bias hold there).  bias may be NULL, nll_s (M x S) may be NULL.
 * Two launches of the NT decoder product over M * Sp rows, neither storing a logit: blm_linear_nll's (lse and nll per row), then
 * the same product with per (token, column tile) partials of sum pbar log pbar and sum_s sum_v p (log p - log pbar) in its
 * epilogue; a fold kernel sums a token's tiles in a fixed order.  One K slice in both: bit-identical run to run in every mode.
 * ws: blm_linear_mc_stats_ws_floats(M, S, V) floats (0: extents out of range), 16-byte aligned, owned by the caller. */
int64_t blm_linear_mc_stats_ws_floats(int M, int S, int V);
int blm_linear_mc_stats(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const int64_t* tgt,
                        int S, float* nll_s, float* bma_nll, float* h_pred, float* mi, float* ws, int M, int V, int K, void* stream);
/* The next-word distribution of the model average, kept: the definitions and the operand layout of blm_linear_mc_stats (x
 * token-major with Sp rows per token, 1 <= S <= 64, w / bias of Np = V rounded up to 4 rows, columns >= V enter nothing, bias
 * may be NULL), and for token m
 *   logp[m,v] = log pbar[v] = log((1/S) sum_s exp(z[s,v] - lse_s)),  v < V      (S = 1: the log-softmax of the row)
 * into the (M, ldo) fp32 buffer logp: ldo >= V, ldo % 4 == 0, 16-byte aligned (BLM_ERR_UNSUPPORTED otherwise); columns >= V of
 * a row (padding) are left unwritten.  h_pred and mi (M each) are optional (NULL: not stored).  tgt is optional too: when given,
 * bma_nll (M, required then) and nll_s (M x S, may be NULL) are filled as blm_linear_mc_stats fills them -- a target outside
 * [0, V) gives NaN for that token's two values only; without tgt both must be NULL.
 * blm_linear_mc_stats' two launches with one more store: pass 2's epilogue forms log pbar = r + L for every (token, column) in
 * registers for the two partial sums anyway, and here each lane also writes its four columns of it (one 16-byte store; the
 * quad that holds column V - 1 of an odd vocabulary stores its real columns one by one).  One K slice, fixed-order folds:
 * bit-identical run to run in every mode.  S * M * V logits are never stored; the M * V result is what a caller samples from,
 * ranks or keeps (bayeslms_amd/incremental.py with mc_samples).
 * ws: blm_linear_mc_logprobs_ws_floats(M, S, V) floats (0: extents out of range), 16-byte aligned, owned by the caller. */
int64_t blm_linear_mc_logprobs_ws_floats(int M, int S, int V);
int blm_linear_mc_logprobs(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const int64_t* tgt,
                           int S, float* logp, int64_t ldo, float* nll_s, float* bma_nll, float* h_pred, float* mi, float* ws,
                           int M, int V, int K, void* stream);
/* Two-model scoring, reference compute_sentence_scores_bayes_jianwei.py:157-168: per-row NLL of the INTERPOLATED logits
 * alpha * (x1 w1^T + b1) + (1 - alpha) * (x2 w2^T + b2) against tgt, as ONE decoder + cross-entropy launch over the packed
 * operands [alpha x1 | (1 - alpha) x2] (M x (K1 + K2)) and [w1 | w2] (N x (K1 + K2)): neither model's (M x N) logits are stored.
 * wcat: blm_linear_nll2_wcat_floats(N, K1, K2) floats, caller-owned; pack_w != 0 (re)builds [w1 | w2] and the mixed bias in it
 * (the first call of a scoring run; later calls with the same weights and alpha pass 0).  ws: blm_linear_nll2_ws_floats floats
 * per call.  K1, K2 and all row strides multiples of 4, operands 16-byte aligned; any N (the packed vocabulary is padded to a
 * multiple of 4 with zero rows whose bias is -inf); b1 / b2 may be NULL.  A target outside [0, N) gives NaN for its row. */
int64_t blm_linear_nll2_wcat_floats(int N, int K1, int K2);
int64_t blm_linear_nll2_ws_floats(int M, int N, int K1, int K2);
int blm_linear_nll2(const float* x1, int64_t ldx1, const float* w1, int64_t ldw1, const float* b1, int K1,
                    const float* x2, int64_t ldx2, const float* w2, int64_t ldw2, const float* b2, int K2, float alpha,
                    const int64_t* tgt, float* nll, float* lse, float* wcat, int pack_w, float* ws, int M, int N, void* stream);

/* N-best rescoring over a prefix trie (compute_scores_batched(share_prefixes=True)), inference only; no reference counterpart.
 * x holds the decoder's input rows of the M trie nodes, edge e = (edge_node[e], edge_tgt[e]) a distinct (node, target) pair:
 *   nll[e] = logsumexp_{v < nv}(x[node,:] . w[v,:] + bias[v]) - (x[node,:] . w[tgt,:] + bias[tgt])
 * without storing the M x N logits: the log-sum-exp per node is blm_linear_nll's launch, the edge's logit a dot product per edge
 * in a fixed order (bit-identical run to run).  w and bias have N rows, N % 4 == 0 (a vocabulary padded once per scoring run);
 * columns >= nv are padding and enter no sum.  bias may be NULL.  An edge whose node is outside [0, M) or whose target is outside
 * [0, nv) gives NaN.  ws: blm_linear_nll_edges_ws_floats(M, N) floats (0: extents out of range), 16-byte aligned, caller-owned. */
int64_t blm_linear_nll_edges_ws_floats(int M, int N);
int blm_linear_nll_edges(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, const int64_t* edge_node,
                         const int64_t* edge_tgt, float* nll, float* ws, int M, int E, int N, int nv, int K, void* stream);
/* The same over two models' INTERPOLATED logits alpha (x1 w1^T + b1) + (1 - alpha) (x2 w2^T + b2), operands and wcat exactly as
 * blm_linear_nll2 takes them (any N; K1, K2 and the row strides multiples of 4, 16-byte aligned operands).
 * ws: blm_linear_nll2_edges_ws_floats(M, N, K1, K2) floats per call. */
int64_t blm_linear_nll2_edges_ws_floats(int M, int N, int K1, int K2);
int blm_linear_nll2_edges(const float* x1, int64_t ldx1, const float* w1, int64_t ldw1, const float* b1, int K1,
                          const float* x2, int64_t ldx2, const float* w2, int64_t ldw2, const float* b2, int K2, float alpha,
                          const int64_t* edge_node, const int64_t* edge_tgt, float* nll, float* wcat, int pack_w, float* ws, int M, int E,
                          int N, void* stream);

/* Kernel-selection options: switches that pick between two BUILT forms of a kernel (each form is parity-tested; the defaults are
 * the measured winners).  Settable at run time; each is initialised from its environment variable on first use.
 *   "attn_hpw"   (BLM_ATTN_HPW,   0) heads per workgroup of the T <= 128 attention kernels: 0 = by head count, 1, 2
 *   "attn_short" (BLM_ATTN_SHORT, 1) one-wave-per-head attention forward for T <= 32 (0: the 128-row forward there too)
 *   "attn_valu"  (BLM_ATTN_VALU,  0) 1: the vector-ALU attention kernels also at head_dim 64
 *   "lstm_gemv"  (BLM_LSTM_GEMV,  1) one-wave-per-unit LSTM step kernel for B <= 4 (0: the matrix-core step kernel)
 *   "lstm_pipe"  (BLM_LSTM_PIPE,  1) software-pipelined K loop of the LSTM step kernels
 *   "lstm_tail"  (BLM_LSTM_TAIL,  0) 1: the general (K tail) form of the pipelined LSTM step kernels also for whole chunks
 *   "lstm_mb2"   (BLM_LSTM_MB2,   1) the architecture-search cell's forward step (blm_lstm_search_step_fwd) takes two batch tiles per
 *                                    workgroup at B > 32: the stacked 8H x H weight streams once, one round of workgroups (0: one tile)
 *   "edit_lane_max" (BLM_EDIT_LANE_MAX, 32) blm_edit_distance: pairs whose shorter sequence has at most this many words (0..32) take
 *                                    the lane-per-pair form, the others the wavefront form (0: every pair with two non-empty sides)
 * and one MODE, off by default:
 *   "deterministic" (BLM_DETERMINISTIC, 0) 1: every reduction of the library in a fixed order -- blm_gemm / blm_linear_nll* plans are
 *                                    legalised to ONE K slice (no float atomics into C; colsum_a then has one writer per element),
 *                                    blm_colsum* / blm_gp_coef_grad use one row chunk, the KL sums of blm_sample_weight /
 *                                    blm_variational_group_fwd / blm_kl_mean_fwd go through block partials added by one block (a
 *                                    fixed array of the code object: these calls must then be issued on one stream at a time),
 *                                    blm_embed_bwd runs one wave per vocabulary row in position order.  Same arithmetic, another
 *                                    order of additions: results equal the default mode's to rounding and are bit-identical run to
 *                                    run (tests/test_gpu_deterministic.py); 1.26-1.33 x the default step time.
 * No reference counterpart (the reference leaves kernel selection to the vendor libraries behind torch). */
/* Diagnostic, no reference counterpart: a bare v_mfma_f32_32x32x2_f32 loop (two waves per SIMD on every CU, no memory traffic),
 * `iters` x 4 MFMAs per wave; *flops receives the work of the launch.  The caller times it (bench.py: "chip.bare_mfma_tflops") --
 * what THIS chip sustains under matrix load, which differs between boxes by up to 10 %.  ws: blm_mfma_probe_ws_floats() floats. */
int64_t blm_mfma_probe_ws_floats(void);
int blm_mfma_probe(float* ws, int iters, double* flops, void* stream);
int blm_set_option(const char* name, int value);
int blm_get_option(const char* name, int* value);

/* Launch plan of a blm_gemm call: block tile (11 = 64x64, 12 = 64x128, 21 = 128x64, 22 = 128x128 rows x cols on four waves;
 * 28 = 128x128 on EIGHT waves: two waves per SIMD in one barrier domain, aligned operands and K % 32 == 0 only) and
 * number of K slices (> 1: partial sums meet in C through float atomics; legal for the plain, bias and Bayesian-wgrad
 * epilogues.  splits <= -2 = TAIL slicing: the tiles of the whole rounds of workgroup slots are computed in one piece with
 * plain stores, only the tiles of the last, partly filled round are cut |splits| ways).  The reference leaves this to the vendor
 * BLAS behind F.linear (model.py:1127-1129); here it is one explicit rule for every shape (csrc/gemm_plan.hip):
 * override > plan table (exact-shape entries measured inside the benchmark / recipe steps, csrc/gemm_plans.inc,
 * written by tools/gemm_tune.py) > cost model (workgroup-slot rounds x per-tile matrix-pipe efficiency).
 * All of this is host code: none of the functions below touches the GPU. */
typedef struct blm_gemm_plan {
  int32_t tile;
  int32_t splits;   /* >= 1: K slices of every tile; <= -2: only the tail round's tiles are sliced, |splits| ways */
  int32_t source;   /* 0 cost model, 1 plan table, 2 override, 3 plan measured beside a collective (comm window open) */
  float model_us;   /* the cost model's estimate for this plan */
} blm_gemm_plan;
/* The plan blm_gemm would use for `a` now (pointers are only inspected for alignment).  A query is not a launch: an open comm
 * window (below) keeps its time. */
int blm_gemm_plan_query(const blm_gemm_args* a, blm_gemm_plan* out);
/* The planning step of a launch on its own: the same plan, AND its modelled time is taken off an open comm window, exactly as
 * blm_gemm / blm_linear_nll do in front of their launch.  For callers that account for matrix work they issue outside the
 * library, and for the host-side tests of the window (tests/test_gemm_plan_cpu.py). */
int blm_gemm_plan_launch(const blm_gemm_args* a, blm_gemm_plan* out);
/* The cost model's estimate (microseconds) of `a` under a given tile / slice count. */
int blm_gemm_plan_model_us(const blm_gemm_args* a, int tile, int splits, float* us);
/* Tuning tools: force a tile and / or a slice count for every call of this process (0 = no override; also read once
 * from BLM_GEMM_TILE / BLM_GEMM_SPLITK). */
int blm_gemm_plan_override(int tile, int splits);
/* Add (or supersede) a plan-table entry at run time; blm_gemm_plan_clear drops the run-time entries and, with
 * keep_builtin == 0, switches the built-in table off as well (cost model only). */
int blm_gemm_plan_set(int op, int M, int N, int K, int epilogue, int accumulate, int tile, int splits);
int blm_gemm_plan_clear(int keep_builtin);
/* Compute units the planner may count on: 0 = the whole chip (256, the default), or 8..256.  Data-parallel training narrows it
 * while gradient buckets are in flight: RCCL's channel workgroups (256 threads, ~280 registers per lane, 19.7 KB LDS each on
 * gfx950) hold CUs beside the backward GEMMs, and a plan that is exactly ONE round of 256 one-per-CU workgroups would spill a
 * second round.  The plan table (measured on the whole chip) applies at 256 only; below it the cost model plans for `cus`.
 * No reference counterpart (single GPU, run_nnlm_ami_tm.sh:44).  blm_gemm_plan_get_cus returns the current value. */
int blm_gemm_plan_set_cus(int cus);
int blm_gemm_plan_get_cus(void);
/* "A gradient bucket is in flight": adds `us` microseconds (the bucket's expected time on the links) to the comm window; every
 * blm_gemm planned while the window is open takes its own modelled time off it, so the window is kept in DEVICE time although
 * the host enqueues far ahead.  Inside the window a launch uses the plan measured beside a resident collective stand-in where
 * the table has one (csrc/gemm_plans_comm.inc, tools/gemm_tune_comm.py; blm_gemm_plan_query reports source 3), its usual plan
 * otherwise.  us = 0 closes the window (engine.GradReducer.finish).  Only launches (and blm_gemm_plan_launch) debit the window.  blm_gemm_plan_set_comm adds a run-time entry to that
 * table (blm_gemm_plan_clear drops the run-time entries of both tables). */
int blm_gemm_plan_comm_window(float us);
float blm_gemm_plan_comm_window_left(void);
int blm_gemm_plan_set_comm(int op, int M, int N, int K, int epilogue, int accumulate, int tile, int splits);

/* --------------------------------------------------------------------------
 * Surrounding Transformer / LSTM ops (HBM-bound unless stated)
 * ------------------------------------------------------------------------ */

/* out[t,b,:] = drop(enc[ids[t,b],:] * scale + pe[t,:])   (model.py:1284,116-117)
 * pe may be NULL (LSTM: plain lookup + dropout, model.py:218).  Dropout keep
 * mask is keyed by the GLOBAL element (t, col_offset + b, j) of a tensor with
 * global_cols columns so that a W-rank run equals a 1-rank run.
 * p == 0 -> no dropout. */
int blm_embed_fwd(const int64_t* ids, const float* enc, const float* pe, float* out, int T, int B, int D,
                  int64_t vocab, float scale, float p, const blm_rng* rng, int col_offset, int global_cols,
                  void* stream);
/* denc[ids[t,b],:] += scale * keep * dy[t,b,:]  (float atomics). */
int blm_embed_bwd(const int64_t* ids, const float* dy, float* denc, int T, int B, int D, int64_t vocab, float scale,
                  float p, const blm_rng* rng, int col_offset, int global_cols, void* stream);

/* out[t,b,:] = drop(x[t,b,:] + pe[t,:])   (PositionalEncoding.forward, model.py:116-117);
 * backward is blm_dropout with the same key. */
int blm_add_pe_dropout(const float* x, const float* pe, float* out, int T, int B, int D, float p, const blm_rng* rng,
                       int col_offset, int global_cols, void* stream);

/* y = x * keep / (1-p)  (nn.Dropout; same call for backward with x = dy).
 * x is (rows, B, D) with the same global-column keying as above. */
int blm_dropout(const float* x, float* y, int rows, int B, int D, float p, const blm_rng* rng, int col_offset,
                int global_cols, void* stream);
/* The same on rows [row0, row0 + rows) of a longer (T, B, D) tensor: x / y point at the block, the keep mask is the one
 * blm_dropout would give those rows (the layer wavefront of a 2-layer LSTM applies the inter-layer dropout chunk by chunk). */
int blm_dropout_rows(const float* x, float* y, int rows, int row0, int B, int D, float p, const blm_rng* rng, int col_offset,
                     int global_cols, void* stream);

/* Post-LN residual block tail (model.py:1041-1042,1044-1045):
 *   s = x + drop(y);  out = LayerNorm(s) * gamma + beta
 * Saves s_out (optional), mean, rstd per row for backward.  D <= 8192. */
int blm_add_dropout_ln_fwd(const float* x, const float* y, const float* gamma, const float* beta, float* out,
                           float* s_out, float* mean, float* rstd, int rows, int B, int D, float eps_ln, float p,
                           const blm_rng* rng, int col_offset, int global_cols, void* stream);
/* Given dout: ds = LN backward wrt s; dx = ds; dy = ds*keep/(1-p);
 * dgamma/dbeta accumulated (+=) via per-block partials in ws
 * (ws >= 2*ceil(M/32)*D floats... see blm_ln_bwd_ws_floats). */
int64_t blm_ln_bwd_ws_floats(int M, int D);
int blm_add_dropout_ln_bwd(const float* dout, const float* s, const float* gamma, const float* mean, const float* rstd,
                           float* dx, float* dy, float* dgamma, float* dbeta, float* ws, int rows, int B, int D,
                           float p, const blm_rng* rng, int col_offset, int global_cols, void* stream);

/* Fused causal self-attention for qkv packed (T, B, 3*d) [q|k|v], head index
 * = b*nhead + head, head_dim = d/nhead (model.py:876-920).  Scaling
 * head_dim^-0.5, additive causal mask, softmax, dropout p on the
 * probabilities, P.V.  Saves lse (B*nhead, T) for backward.  Any T and any
 * head_dim <= 512 are taken; which kernels run: head_dim 64 -- matrix cores
 * (T <= 128 one tile, longer sequences chunked); 4 / 8 / 16 / 32 at T <= 128 --
 * vector ALU, a query per lane; any other head_dim <= 128 at T <= 128 -- vector
 * ALU, two lanes per row; everything else -- one wave per query, untiled.
 * q/k/v may also be three separate (T,B,d) tensors (BayesMultiheadAttention,
 * model.py:975-977): pass ld_qkv = d. */
int blm_attn_fwd(const float* q, const float* k, const float* v, int64_t ld_qkv, float* out, float* lse, int T, int B,
                 int nhead, int head_dim, float p, const blm_rng* rng, int col_offset, int global_cols, void* stream);
int blm_attn_bwd(const float* q, const float* k, const float* v, int64_t ld_qkv, const float* out, const float* dout,
                 const float* lse, float* dq, float* dk, float* dv, int64_t ld_dqkv, int T, int B, int nhead,
                 int head_dim, float p, const blm_rng* rng, int col_offset, int global_cols, void* stream);
/* Inference on PACKED rows (the n-best scorer keeps only the real tokens of a padded (T, B) batch of hypotheses through the whole
 * Transformer stack): q / k / v are (R, ld_qkv) and out (R, nhead * head_dim) matrices of the R real tokens, rowmap (T * B) int32
 * gives the row of the token at padded position t * B + b or -1 for padding (the real tokens of a column are a prefix of it).
 * Same arithmetic as blm_attn_fwd without dropout; nothing is scattered to or gathered from a padded buffer.  head_dim 64 and
 * T <= 32 (one wave per head); anything else returns BLM_ERR_UNSUPPORTED and the caller scatters / gathers around blm_attn_fwd. */
int blm_attn_fwd_rows(const float* q, const float* k, const float* v, int64_t ld_qkv, float* out, const int32_t* rowmap, int T,
                      int B, int nhead, int head_dim, void* stream);
/* Inference over the R nodes of prefix tries (the n-best scorer with shared prefixes): q / k / v are (R, ld_qkv) and out
 * (R, nhead * head_dim) matrices of the nodes in DFS preorder, each utterance's nodes contiguous; row i attends row j iff
 * lo[i] <= j <= i and end[j] > i (j is i or an ancestor of i: end[j] is one past j's subtree, lo[i] the first node of i's
 * utterance).  Same scaling and softmax as blm_attn_fwd without dropout; a row that attends no key gives NaN.  head_dim 64 --
 * matrix cores, 128-query tiles of the flat row range walking the key chunks from their smallest lo (attention_mfma.hip);
 * any other head_dim <= 128 -- vector ALU, one wave per query walking its path; larger head sizes return BLM_ERR_UNSUPPORTED. */
int blm_attn_fwd_tree(const float* q, const float* k, const float* v, int64_t ld_qkv, float* out, const int32_t* end, const int32_t* lo,
                      int R, int nhead, int head_dim, void* stream);
/* The same backward with a caller-owned scratch buffer of blm_attn_bwd_ws_floats() floats (0: this shape has no use
 * for one): the dK/dV kernel leaves dS (B*nhead, T, T) there and dQ = dS K is one small product instead of a second
 * recomputation of the probabilities and their dropout masks.  ws == NULL is blm_attn_bwd.  Same results. */
int64_t blm_attn_bwd_ws_floats(int T, int B, int nhead, int head_dim);
int blm_attn_bwd_ws(const float* q, const float* k, const float* v, int64_t ld_qkv, const float* out, const float* dout,
                    const float* lse, float* dq, float* dk, float* dv, int64_t ld_dqkv, int T, int B, int nhead,
                    int head_dim, float p, const blm_rng* rng, int col_offset, int global_cols, float* ws,
                    int64_t ws_floats, void* stream);
/* The same attention with the dropout factors of the probabilities HANDED OVER instead of generated from the Philox stream: keep is
 * (global_cols * nhead, T, T) floats, 0 or 1 / (1 - p), indexed by the head ((col_offset + b) * nhead + head) as the reference's
 * (B * h, T, T) probability tensor is (model.py:905-914: softmax -> nn.Dropout -> bmm).  A parity path -- the caller passes the mask
 * torch's CPU dropout drew (NoiseState.source "torch"); always the vector-ALU kernels, any head size / length. */
int blm_attn_fwd_keep(const float* q, const float* k, const float* v, int64_t ld_qkv, float* out, float* lse, int T, int B, int nhead,
                      int head_dim, const float* keep, int col_offset, int global_cols, void* stream);
int blm_attn_bwd_keep(const float* q, const float* k, const float* v, int64_t ld_qkv, const float* out, const float* dout,
                      const float* lse, float* dq, float* dk, float* dv, int64_t ld_dqkv, int T, int B, int nhead, int head_dim,
                      const float* keep, int col_offset, int global_cols, void* stream);

/* --------------------------------------------------------------------------
 * Incremental decoding with a key/value cache (bayeslms_amd/incremental.py; csrc/decode.hip).  New: the reference rescoring and
 * training scripts have no such path.  Inference only, no dropout, vector ALU throughout.
 *
 * Cache layout, one fp32 allocation per state: [layer][k|v][stream < n_cap][head][t < max_len][head_dim] -- each (stream, head)
 * owns a contiguous max_len x head_dim panel.  `kv` below is one layer's block (K panels, then the V panels
 * n_cap * nhead * max_len * head_dim floats later).  `past` (N,) int32: tokens already in each stream's panels.  `n_new` (N,)
 * int32 (NULL: Tq for every stream): the real rows of a ragged chunk, rows t >= n_new[n] are padding.
 * ------------------------------------------------------------------------ */

/* Causal attention of Tq new query rows per stream over the cache: row (t, n) attends cache positions [0, past[n] + t], its own
 * key included (blm_kv_append it first).  q is (Tq, N, ld_q) -- head h at columns [h * head_dim, (h + 1) * head_dim), so the fused
 * [q|k|v] projection passes as it is; out is (Tq, N, nhead * head_dim), zeros on padding rows.  Scaling and softmax of
 * blm_attn_fwd without dropout.  Split-K flash decoding: workgroups over (key chunk of 64, stream * head, 16 query rows) leave
 * per-chunk (max, sum, P.V) partials in ws, a second launch combines them in chunk order (no atomics: bitwise repeatable).
 * ctx_max: an upper bound of past[n] + n_new[n] over the streams (the caller's host mirror of the lengths); it sizes the grid and
 * the workspace, keys at positions >= ctx_max are never read.  ws: blm_attn_decode_ws_floats(Tq, N, nhead, ctx_max, head_dim)
 * floats (0: out of range).  head_dim 1..128 (BLM_ERR_UNSUPPORTED beyond). */
int64_t blm_attn_decode_ws_floats(int Tq, int N, int nhead, int ctx_max, int head_dim);
int blm_attn_decode(const float* q, int64_t ld_q, const float* kv, const int32_t* past, const int32_t* n_new, float* out, float* ws,
                    int64_t ws_floats, int Tq, int N, int n_cap, int nhead, int max_len, int head_dim, int ctx_max, void* stream);
/* kv[k|v][n][h][past[n] + t][:] = k / v[t, n, h * head_dim : (h + 1) * head_dim] for t < n_new[n] (positions >= max_len are not
 * written); k / v are (Tq, N, ld_kv) strided views (of the fused projection).  `past` is not advanced: the caller owns it. */
int blm_kv_append(const float* k, const float* v, int64_t ld_kv, float* kv, const int32_t* past, const int32_t* n_new, int Tq, int N,
                  int n_cap, int nhead, int max_len, int head_dim, void* stream);
/* Beam prune / fork, every layer and both K and V in ONE launch: new stream j continues old stream idx[j] (int64, may repeat;
 * entries outside [0, n_src) copy nothing).  State = `outer` blocks of [stream < n_cap][head][max_len][head_dim]; only the live
 * prefix len[idx[j]] of each panel is copied (len NULL: whole panels), and len_out[j] = len[idx[j]] when len_out is given.
 * KV caches: outer = 2 * layers.  LSTM (h, c) rows: outer = 2 * layers, nhead = max_len = 1, head_dim = H, len NULL.  Source and
 * destination states may not overlap (BLM_ERR_INVALID: double-buffer the state). */
int blm_kv_gather(const float* src, float* dst, const int64_t* idx, const int32_t* len, int32_t* len_out, int M, int n_src, int n_cap,
                  int outer, int nhead, int max_len, int head_dim, void* stream);
/* out[t, n, :] = (ids ? enc[ids[t, n]] * scale : x[t, n, :]) + (pe ? pe[pos0[n] + t] : 0) -- PositionalEncoding.embed / .forward
 * (model.py:1284,116-117) at per-stream offsets, eval mode.  A row whose id or position is out of range is NaN. */
int blm_embed_at(const int64_t* ids, const float* enc, int64_t vocab, float scale, const float* x, const float* pe, int pe_rows,
                 const int32_t* pos0, float* out, int Tq, int N, int D, void* stream);
/* out[r, :V] = x[r, :V] - logsumexp(x[r, :V]); row strides ldx / ldo >= V (padded vocabulary rows); in place when out == x and
 * ldo == ldx, any other overlap of x and out is refused. */
int blm_log_softmax_rows(const float* x, int64_t ldx, float* out, int64_t ldo, int R, int V, void* stream);
/* One id per row of x (R, V; row stride ldx).  temperature 0: argmax, lowest index on ties.  Otherwise Gumbel-max over
 * x / temperature with u from Philox: counter (column, row, rng->stream, rng->step), key rng->seed, first word;
 * u = ((w >> 8) + 0.5) * 2^-24, noise -log(-log u).  The same rng gives the same ids. */
int blm_sample_rows(const float* x, int64_t ldx, int R, int V, float temperature, const blm_rng* rng, int64_t* out, void* stream);
/* What an evaluation needs of each row of x (R, V; row stride ldx >= V), logits or log-probabilities alike -- the row is
 * normalised here, read ONCE (csrc/rowstats.hip).  With lse = logsumexp(x[r, :V]) and p = softmax(x[r, :V]):
 *   nll[r] = lse - x[r, tgt[r]];  conf[r] = exp(max - lse), the largest p;  entropy[r] = lse - sum_v p_v x_v (a column at -inf
 *   adds 0);  pred[r] = the lowest index that holds the maximum;  rank[r] = the columns strictly greater than the target's
 *   value + the equal ones at a lower index (0: the target is the prediction).
 * A target outside [0, V) gives nll NaN and rank -1 in that row only; a row that holds a NaN gives nll = conf = entropy = NaN and
 * pred = rank = -1.  Every output pointer may be NULL; tgt may be NULL, and nll and rank must then be NULL too.  Folds run in a
 * fixed order without atomics: the same bits in every run.  No workspace. */
int blm_row_stats(const float* x, int64_t ldx, const int64_t* tgt, int R, int V, float* nll, float* conf, float* entropy,
                  int32_t* pred, int32_t* rank, void* stream);
/* blm_row_stats at several temperatures from the same single read of x (temperature scaling: engine.evaluate_temperatures,
 * engine.fit_temperature).  For an inverse temperature b = 1 / T > 0 the tempered distribution of a row is p_b ~ exp(b x) --
 * for a row of log pbar that is pbar^b / Z.  With m = max x, d = x - m, s = sum exp(b d) and r = sum exp(b d) d / s = E_b[x] - m:
 *   nll = b (m - x[tgt]) + log s;  conf = 1 / s;  entropy = log s - b r;  dnll = d nll / d b = (m - x[tgt]) + r.
 * pred and rank are blm_row_stats' and do not depend on b.  The list travels in this host struct, read before the launch and
 * handed to the kernel by value: no device memory, no copy. */
#define BLM_ROW_TEMPS_MAX 8
typedef struct blm_row_temps {
  uint32_t abi_version; /* BLM_ABI_VERSION */
  int32_t count;        /* 1 .. BLM_ROW_TEMPS_MAX */
  float beta[BLM_ROW_TEMPS_MAX]; /* beta[j] finite and > 0 for j < count; the others are not read */
} blm_row_temps;
/* x, ldx, tgt, R, V as for blm_row_stats.  nll / conf / entropy / dnll: (count, R) contiguous, temperature j's figure of row r
 * at [j * R + r], each may be NULL; pred / rank (R), each may be NULL; nll, dnll and rank need tgt.  Kernel forms exist for 1,
 * 2, 4 and 8 temperatures, a count in between runs the next larger one with its surplus slots idle and unwritten.  The figures
 * of beta[j] are bit-identical whatever else the list holds and wherever in the list it stands, and the same in every run.  A
 * row that holds a NaN, a target outside [0, V) and a target at -inf (nll = dnll = +inf) are answered as blm_row_stats answers
 * them, in every temperature's slot.  BLM_ERR_INVALID, before any launch: NULL x or temps, count outside
 * 1..BLM_ROW_TEMPS_MAX, a beta that is not finite or not > 0, R < 0, V <= 0, ldx < V, nll / dnll / rank without tgt, extents too
 * large; BLM_ERR_ABI: abi_version.  R == 0: BLM_OK, nothing launched.  No workspace. */
int blm_row_stats_temps(const float* x, int64_t ldx, const int64_t* tgt, int R, int V, const blm_row_temps* temps, float* nll,
                        float* conf, float* entropy, float* dnll, int32_t* pred, int32_t* rank, void* stream);

/* --------------------------------------------------------------------------
 * Continuous neural cache (csrc/cache.hip; Grave, Joulin, Usunier, ICLR 2017): a pointer distribution over recent hidden
 * states.  Row i of a text has the decoder input h_i and the target y_i, the word that followed; with a window N, theta >= 0
 * and C_t = { i : max(0, t - N) <= i < t }:
 *   lse[t]   = log sum_{i in C_t}            exp(theta h_t . h_i)      (-inf: C_t is empty)
 *   match[t] = log sum_{i in C_t, y_i = y_t} exp(theta h_t . h_i)      (-inf: no key matches)
 *   p_cache(y_t) = exp(match - lse);   p(y_t) = (1 - lambda) p_model(y_t) + lambda p_cache(y_t),  0 <= lambda < 1;
 *   an empty cache takes p = p_model.
 * The entry point is the general banded form: M queries q (row stride ldq >= K), Nk keys k (row stride ldk >= K) with
 * label[i], a target tgt[m] per query, and per query the key range [max(lo[m], hi[m] - window, 0), min(hi[m], Nk)) -- lo and hi
 * are DEVICE arrays, clamped by the kernel: whatever they hold, nothing outside k and label is read, and a reversed or empty
 * range gives -inf in both outputs.  lo may be NULL (= 0).  The evaluation passes q = k = the text's rows and hi[t] = t.
 * Labels and targets are compared as 64-bit integers, nothing else is asked of them.
 * The dot products run on the fp32 matrix cores; the scores are reduced on chip (one running maximum of the raw score serves
 * every theta), never stored; only key tiles between the least start and the greatest end of a workgroup's 128 queries are
 * visited.  A matching key whose weight underflows float32 beside the range's maximum (theta (max - score) > 87) leaves match
 * at -inf.  The figures of theta[j] are those of a launch with theta[j] alone up to rounding, and the same bits in every run.
 * -------------------------------------------------------------------------- */
#define BLM_CACHE_THETAS_MAX 8
typedef struct blm_cache_thetas {
  uint32_t abi_version; /* BLM_ABI_VERSION */
  int32_t count;        /* 1 .. BLM_CACHE_THETAS_MAX */
  float theta[BLM_CACHE_THETAS_MAX]; /* theta[j] finite and >= 0 for j < count; the others are not read */
} blm_cache_thetas;
/* lse / match: (count, M) contiguous, theta j's figure of query m at [j * M + m].  Kernel forms exist for 1, 2, 4 and 8
 * thetas, a count in between runs the next larger one with its surplus slots idle and unwritten.  ws: unused, may be NULL (no
 * workspace: nothing leaves the registers but the two log-sums).  BLM_ERR_INVALID, before any launch: NULL q, k, label, tgt,
 * hi, thetas, lse or match; count outside 1..BLM_CACHE_THETAS_MAX; a theta that is negative or not finite; M < 0, Nk < 0,
 * K < 1, ldq < K, ldk < K, window < 1, extents too large; BLM_ERR_ABI: abi_version.  M == 0: BLM_OK, nothing launched. */
int blm_cache_scores(const float* q, int64_t ldq, const float* k, int64_t ldk, const int64_t* label, const int64_t* tgt,
                     const int32_t* lo, const int32_t* hi, int window, int M, int Nk, int K, const blm_cache_thetas* thetas,
                     float* lse, float* match, float* ws, void* stream);

/* --------------------------------------------------------------------------
 * Dynamic evaluation (csrc/dyneval.hip; Krause, Kahembwe, Murray, Renals, ICML 2018): the weights adapt to the text while it is
 * scored.  The text is laid out as the evaluation lays it out, in columns, and walked in windows of seq_len rows, ONE window at
 * a time (no grouping of windows: a window must not see weights adapted on its own future); all columns share one set of
 * weights (one column is the paper's setting).  For window k with weights theta_k (theta_0 = theta*, the trained weights):
 *   1. score     eval mode (mean weights, no dropout, no noise), grad enabled; NLL_k, the per-token NLL of the window under
 *                theta_k, is what the report sums.  An LSTM's state is carried and detached between windows, a Transformer's
 *                windows are independent, as in the static evaluation.
 *   2. gradient  g = gradient of the window's MEAN NLL over its tokens.  No KL term, no clip.
 *   3. update    none after the last window; element-wise over every trainable parameter
 *        sgd rule (no statistics):  theta <- theta - eta g                     + min(1, lambda)          (theta* - theta)
 *        rms rule:                  theta <- theta - eta g / (r + eps rbar)    + min(1, lambda r / rbar) (theta* - theta)
 *        r_i = sqrt(MS_i), MS_i the mean of g_i^2 over the statistics windows; rbar the mean of r over the LIVE entries, those
 *        with MS_i > 0 (in eval mode log sigma never receives a gradient and a flat buffer has padding: neither may dilute
 *        rbar).  eps is RELATIVE to rbar (the paper's absolute epsilon is eps rbar): it bounds the step of an entry the
 *        statistics never saw, such as an embedding row absent from the statistics text, to 1 / eps average steps whatever the
 *        scale of the gradients.
 *   4. statistics  steps 1-2 on another text (the training text) for its first W windows with NO update; MS = sum of g^2 / W.
 * In fp32 the update is evaluated as exactly  p - step + d * (p0 - p)  without contraction, with
 *   sgd: step = lr * g,                                     d = min(1, decay)
 *   rms: step = g == 0 ? 0 : (lr * g) / (r + eps * rbar),   d = min(1, (decay / rbar) * r)
 * (eps * rbar and decay / rbar rounded once per launch), so an entry with g = 0 and p = p0 keeps its bits under either rule.
 *
 * The three entry points work on flat arrays of n floats (one call covers a whole model held in one flat buffer; no pointer
 * table).  Arrays that are 16-byte aligned take 16-byte loads and stores over the body and a scalar tail; any other alignment
 * (of a float) is ACCEPTED and takes the scalar path for the whole array.  BLM_ERR_INVALID, before any launch: a NULL array,
 * n < 0 or n > 2^40, count < 1, lr / decay / eps negative or not finite, rms given without mean or mean without rms, ws not
 * 8-byte aligned.  n == 0: BLM_OK (blm_dyneval_rms still writes mean = {0, 0}).
 * -------------------------------------------------------------------------- */
/* floats of workspace blm_dyneval_rms needs (two doubles per workgroup of its first stage), 8-byte aligned */
#define BLM_DYNEVAL_RMS_WS_FLOATS 4096
/* ms[i] += g[i]^2 */
int blm_dyneval_accum(float* ms, const float* g, int64_t n, void* stream);
/* rms[i] = sqrt(ms[i] / count); mean (DEVICE float[2]) = { rbar = mean of rms over the entries with ms > 0 (0 without one), the
 * number of those entries as a float (exact up to 2^24, rounded beyond) }.  The partial sums are doubles, added in two stages
 * in a fixed order without atomics: the same bits in every run, deterministic option or not.  rms must not overlap ms. */
int blm_dyneval_rms(const float* ms, int64_t n, int count, float* rms, float* mean, float* ws, void* stream);
/* One grid-stride pass over p (updated in place), g, p0 and, for the rms rule, rms.  rms == NULL and mean == NULL: the sgd rule
 * (eps unused).  mean is the DEVICE pair blm_dyneval_rms wrote: rbar is read on the device, so a walk needs no host
 * synchronisation; it must be > 0 (a statistics run without a live entry is the caller's error to report).  zero_grad != 0
 * also writes g = 0 in the same pass.  p, g, p0 and rms must not overlap one another. */
int blm_dyneval_update(float* p, float* g, const float* p0, const float* rms, const float* mean, int64_t n, float lr, float decay,
                       float eps, int zero_grad, void* stream);

/* --------------------------------------------------------------------------
 * SWAG (csrc/swag.hip; Maddox, Garipov, Izmailov, Vetrov, Wilson, NeurIPS 2019): a Gaussian over ALL weights fitted to the SGD
 * iterates, and the model average over its samples.  P floats of weights in one flat buffer, n iterates collected so far, a
 * ring of K <= BLM_SWAG_RANK_MAX deviation rows.
 *
 * Collection of iterate theta as number n (count = n), Welford form (no sq - mean^2 cancellation), in fp32 in this order and
 * without contraction, inv = 1 / (n + 1) rounded once:
 *   d = theta - mean;  mean' = mean + d * inv;  dev = theta - mean';  m2' = m2 + d * dev
 * and dev goes to row n mod K of the ring (the caller passes that row).  count == 0 writes mean' = theta, m2' = 0, dev = 0 and
 * reads neither mean nor m2, which may be uninitialised.  var = m2 / n is the population variance; K_live = min(n, K).
 *
 * Sample j:  theta_j = mean + a sqrt(max(var, floor)) z1_j + b sum_{k < K_live} D[k] z2[j][k], evaluated in fp32 as
 *   sd = a * sqrt(max(m2 * inv_n, floor));  base = fma(sd, z1, mean);  low = fma(D[k], z2[j][k], low), k ascending from low = 0;
 *   out = fma(b, low, base)
 * with a, b, inv_n = 1 / n and floor rounded to fp32 once by the caller (full form, K_live >= 2: a = sqrt(c / 2),
 * b = sqrt(c / (2 (K_live - 1))) for a scale c; diagonal form: a = sqrt(c), k_live = 0).  z1_j[i] is element i of the Philox
 * normal stream (rng.seed, rng.stream, step = sample_id[j]): the values blm_philox_normal writes for that blm_rng; rng.step is
 * not read.  By convention rng.stream = BLM_STREAM_SWAG + 0 and z2[j][.] are the first K_live elements of
 * (seed, BLM_STREAM_SWAG + 1, step = sample_id[j]).  A sample is a pure function of (mean, m2, D, seed, id, a, b, inv_n, floor):
 * the same bits alone, in a longer list, at another slot and on either the 16-byte or the scalar path.
 *
 * Average of the S samples' next-word distributions, row by row: for sample s with logits z_s,
 *   logp_s = z_s - lse(z_s);  acc = log((1 / S) sum_s exp(logp_s));  H_s = -sum_v p_s log p_s;  hsum = sum_s H_s
 * accumulated one sample per call: s == 0 writes acc = logp_0 and hsum = H_0 without reading either, every later s folds
 * acc = max(acc, logp) + log1p(exp(-|acc - logp|)) (both -inf: -inf), and s == S - 1 then subtracts log S.
 * -------------------------------------------------------------------------- */
#define BLM_SWAG_RANK_MAX 32
#define BLM_SWAG_DRAWS_MAX 8
#define BLM_SWAG_SAMPLES_MAX 64
typedef struct blm_swag_draw {
  uint32_t abi_version; /* BLM_ABI_VERSION */
  int32_t count;        /* 1 .. BLM_SWAG_DRAWS_MAX samples in this launch */
  float a, b;           /* finite, >= 0 */
  float inv_n;          /* 1 / n: finite, > 0 */
  float var_floor;      /* the floor under var: finite, >= 0 */
  uint32_t sample_id[BLM_SWAG_DRAWS_MAX]; /* sample_id[j] for j < count; the others are not read */
  blm_rng rng;          /* seed and stream of z1; step is not read (sample_id[j] takes its place) */
} blm_swag_draw;
/* One streaming pass.  dev_row == NULL: diagonal posterior, no deviation is written.  Arrays that are 16-byte aligned take
 * 16-byte accesses over the body and a scalar tail; any other alignment of a float takes the scalar path whole.  The arrays must
 * not overlap.  BLM_ERR_INVALID, before any launch: NULL theta, mean or m2, n_floats outside 0..2^40, count outside 0..2^24-1.
 * n_floats == 0: BLM_OK. */
int blm_swag_collect(const float* theta, float* mean, float* m2, float* dev_row, int64_t n_floats, int64_t count, void* stream);
/* out: draw->count rows of n_floats at stride ld_out; dev: k_live rows at stride ld_dev; z2: draw->count rows of k_live floats,
 * contiguous, on the device (NULL with k_live == 0, as dev).  A count of 3 or 5..7 runs the form of 4 or 8 slots with the surplus
 * slots idle: nothing is computed or written for them.  All slots come from one read of mean, m2 and the deviation rows.
 * BLM_ERR_INVALID, before any launch: NULL out, mean, m2 or draw, count outside 1..BLM_SWAG_DRAWS_MAX, k_live outside
 * 0..BLM_SWAG_RANK_MAX, k_live > 0 without dev or z2, ld_out or ld_dev < n_floats, n_floats outside 0..2^40, a / b / floor negative
 * or not finite, inv_n not finite or not > 0; BLM_ERR_ABI: abi_version.  n_floats == 0: BLM_OK. */
int blm_swag_sample(float* out, int64_t ld_out, const float* mean, const float* m2, const float* dev, int64_t ld_dev, int k_live,
                    const float* z2, int64_t n_floats, const blm_swag_draw* draw, void* stream);
/* logits (rows, V) at row stride ld, acc (rows, V) at row stride ld_acc, not overlapping.  hsum (rows,) may be NULL.  targets
 * (rows,) int64 and nll_s (S, rows) go together or are both NULL: nll_s[s * rows + r] = -logp_s[r, targets[r]], and 0 for a
 * target outside [0, V), as in blm_ce_fwd_bwd.  One workgroup per row: rows held in registers for V <= 36864 when both bases
 * are 16-byte aligned and both strides multiples of 4, two sweeps otherwise.  No atomics, fixed order.
 * BLM_ERR_INVALID, before any launch: NULL logits or acc, targets without nll_s or the reverse, rows < 0, V <= 0, ld or ld_acc
 * < V, S outside 1..BLM_SWAG_SAMPLES_MAX, s outside [0, S), extents too large.  rows == 0: BLM_OK. */
int blm_logp_avg_accum(const float* logits, int64_t ld, float* acc, int64_t ld_acc, const int64_t* targets, int rows, int V, int s,
                       int S, float* hsum, float* nll_s, void* stream);

/* --------------------------------------------------------------------------
 * Stochastic-gradient MCMC (csrc/sgmcmc.hip; bayeslms_amd/sgmcmc.py): one weight update of stochastic-gradient Langevin
 * dynamics (Welling and Teh, ICML 2011) or of its RMSprop-preconditioned form (Li, Chen, Carlson, Carin, AAAI 2016; on LSTM
 * language models: Gan, Li, Chen, Pu, Su, Carin, ACL 2017) over n floats of weights in one flat buffer.
 *
 * Per element i, in fp32, in exactly this order and without contraction (every product and sum below is one rounded operation,
 * evaluated left to right inside the parentheses shown):
 *   c  = min(1, clip / (sqrt(sq) * grad_scale + 1e-6)) * grad_scale          (blm_clip_sgd_multi's clip; once per lane)
 *   d  = (c * g[i]) + (weight_decay * p[i])
 *   sgld   (v == NULL):  p[i] = (p[i] - lr * d) + sigma * xi[i]
 *   psgld  (v != NULL):  v[i] = (alpha * v[i]) + ((1 - alpha) * d) * d,      1 - alpha rounded once by the launcher
 *                        G    = 1 / (damping + sqrt(v[i]))                   with the NEW v[i]
 *                        p[i] = (p[i] - (lr * G) * d) + (sigma * sqrt(G)) * xi[i]
 * sqrt and the division are correctly rounded.  xi[i] is element i of the Philox normal stream (rng.seed, rng.stream, rng.step):
 * the values blm_philox_normal writes for that blm_rng.  By convention rng.stream = BLM_STREAM_SGMCMC and rng.step is the
 * optimisation step.  i is the index into the array handed in, whatever the launch geometry and whichever path an element
 * takes: 16-byte aligned arrays take 16-byte loads and stores over the body and a scalar tail, any other alignment of a float is
 * ACCEPTED and takes the scalar path whole, and an element gets the same bits either way.  sigma == 0 adds no noise term at all
 * (the generator does not run, rng may be NULL), so with weight_decay = 0 the sgld rule is blm_clip_sgd_multi at momentum 0 up
 * to that kernel's contraction.  An entry with g = 0, p = 0 (and v = 0) moves by the noise alone: G = 1 / damping there.
 *
 * The term Gamma(theta) of Li et al. (the derivative of the preconditioner, their eq. 3) is DROPPED, as in their practical
 * algorithm, which argues that the term is small for alpha near 1.  Clipping biases the chain as well.
 *
 * sq is the DEVICE scalar blm_sqnorm_multi leaves (the squared norm of g before grad_scale).  p, g and v must not overlap.
 * No atomics and no reductions: the same bits in every run.
 * BLM_ERR_INVALID, before any launch: NULL p, g or sq; n outside 0..2^40; clip not > 0; lr, sigma or weight_decay negative or
 * not finite; with v: alpha outside [0, 1) or damping not > 0; rng == NULL with sigma > 0.  n == 0: BLM_OK.
 * -------------------------------------------------------------------------- */
int blm_sgmcmc_update(float* p, const float* g, float* v, const float* sq, int64_t n, float clip, float lr, float grad_scale,
                      float weight_decay, float sigma, float alpha, float damping, const blm_rng* rng, void* stream);

/* --------------------------------------------------------------------------
 * Last-layer Laplace posterior for the decoder (csrc/laplace.hip; bayeslms_amd/laplace.py; MacKay 1992; Kristiadi, Hein, Hennig
 * 2020; Daxberger et al. 2021): a Gaussian over the decoder's weights fitted after training, from one pass over a text.
 *
 * Decoder: z = W h + b with W (V, K) at the trained (mean) weights, p = softmax(z).  Prior N(0, 1/tau I), 0 < tau <= inf.
 * Posterior precision, the diagonal of the generalised Gauss-Newton matrix summed over the N rows of a fit text:
 *   a_t[v] = p_t[v] (1 - p_t[v]);   F_W[v,k] = sum_t a_t[v] h_t[k]^2;   F_b[v] = sum_t a_t[v];   Lambda = F + tau.
 * No label enters: every row of the fit text counts, whatever its target.
 * Predictive logits of a new row h: mean z, variance var[v] = sum_k h[k]^2 / Lambda_W[v,k] + 1 / Lambda_b[v] -- under a diagonal
 * posterior exactly diagonal over v.  tau = inf gives var = 0, the model itself.
 * Three links from (z, var) to a next-word distribution:
 *   probit  ptilde = softmax(z / sqrt(1 + (pi / 8) var)), the mean-field approximation.  NOT invariant to a shift of the logits
 *           z + c: the result depends on where the decoder's bias happens to put the row.
 *   expexp  ptilde = softmax(z + var / 2) = E[e^{z_v}] / sum_u E[e^{z_u}].  Shift-invariant.
 *   mc      S samples, the estimate the two closed forms approximate and the only link with a mutual information:
 *             z_s[v] = fma(sqrt(var[v]), eps_s[v], z[v]);  p_s = softmax(z_s);  pbar = (1/S) sum_s p_s;
 *             bma_nll = -log pbar[t];  h_pred = -sum_v pbar log pbar;  mi = (1/S) sum_s sum_v p_s (log p_s - log pbar), the KL
 *             form of blm_linear_mc_stats, never a difference of two entropies;  conf = max_v pbar, pred the lowest index that
 *             holds it, rank that of the target under pbar;  nll_s[s] = lse_s - z_s[t].
 * Noise: eps_s[r, v] is element ((row0 + r) Vq + v) of the Philox normal stream (seed, BLM_STREAM_LAPLACE, step = s), Vq = V
 * rounded up to 4: the values blm_philox_normal writes; row0 is the global index of the chunk's first row.  A token's figures
 * therefore do not depend on how the text was chunked, on S, or on which other samples run beside it.
 *
 * The three entry points: vector ALU, one workgroup per row, folds in a fixed order without atomics (the same bits in every
 * run), 16-byte accesses where bases are 16-byte aligned and strides multiples of 4, a guarded scalar path otherwise.  No
 * workspace.  BLM_ERR_INVALID before any launch: a NULL operand, a negative count, V <= 0, a row stride below V, extents too
 * large, and what each entry adds below.  Zero rows: BLM_OK, nothing launched.
 * -------------------------------------------------------------------------- */
#define BLM_LAPLACE_SAMPLES_MAX 32
/* a[r, v] = fma(-p, p, p) with p = exp(x - lse) of row r of logits (rows, V; row stride ld), v < V; columns V .. Vq - 1 of a are
 * written 0 when lda >= Vq.  a == logits with lda == ld is in place; any other overlap is refused.  One read of the row, one
 * write, for V <= 36864 on the 16-byte path (the row is held in registers); two sweeps of the row otherwise.  A column at -inf
 * gives 0; a row that holds a NaN gives a NaN row. */
int blm_laplace_curvature(const float* logits, int64_t ld, float* a, int64_t lda, int rows, int V, void* stream);
/* blm_row_stats' five figures of y[v] = link(z[r, v], var[r, v]) -- link 0: probit, 1: expexp -- with its rules for ties, NULL
 * outputs and targets, and vbar[r] = sum_v ptilde_v var_v, a per-token variance figure (may be NULL).  z and var (R, V; row
 * strides ldz, ldv) are each read once; y is formed in registers and never stored.  The probit's reciprocal square root is the
 * hardware's (1 ulp).  A row with a NaN, or with a var that is negative, NaN or infinite, is answered as blm_row_stats answers
 * a NaN row (vbar NaN too); a target outside [0, V) as there.  BLM_ERR_INVALID also: another link, nll or rank without tgt. */
int blm_laplace_row_stats(const float* z, int64_t ldz, const float* var, int64_t ldv, const int64_t* tgt, int R, int V, int link,
                          float* nll, float* conf, float* entropy, int32_t* pred, int32_t* rank, float* vbar, void* stream);
/* The mc link over S samples, 1 <= S <= BLM_LAPLACE_SAMPLES_MAX; rng gives seed and stream, rng->step is not read.  Outputs are
 * (R,), nll_s is (S, R) with sample s of row r at [s * R + r]; each may be NULL; bma_nll, nll_s and rank need tgt.  Nothing of
 * S x V reaches memory: the noise is made in registers and made again wherever a later sweep needs it (three times in all).
 * Sweep 1 finds lse_s, eight samples per pass over the row (z and var come from HBM once, the later passes re-read a row the
 * workgroup just streamed); sweep 2 forms pbar of a column, then that column's KL terms.  One form for every V.  In fp32:
 * sd = sqrt(var), pbar = (sum_s exp(z_s - lse_s)) * (1 / S), s ascending; sample s runs the same operations whatever S is.
 * A row with a NaN or with a var that is negative, NaN or infinite gives NaN in every float output and -1 in pred and rank; a
 * target outside [0, V) gives NaN in bma_nll and nll_s and -1 in rank for that row only.  BLM_ERR_INVALID also: S out of
 * range, row0 outside 0..2^40. */
int blm_laplace_mc_rows(const float* z, int64_t ldz, const float* var, int64_t ldv, const int64_t* tgt, int R, int V, int S,
                        const blm_rng* rng, int64_t row0, float* bma_nll, float* nll_s, float* h_pred, float* mi, float* conf,
                        int32_t* pred, int32_t* rank, void* stream);

/* --------------------------------------------------------------------------
 * Word error rate of rescored n-best lists (csrc/nbest.hip; bayeslms_amd/nbest_wer.py): word-level alignment in bulk, selection
 * over a grid of score weights, minimum-Bayes-risk selection (Stolcke, Koenig, Weintraub 1997).
 *
 * Sequences are int32 word ids in one flat buffer tok (n_tok words); off holds n_seq + 1 int64 offsets, sequence q is
 * tok[off[q] .. off[q + 1]).  The ids are the caller's, assigned from the SURFACE words of hypotheses and references together
 * (not an LM vocabulary: an out-of-vocabulary word must not collapse to <unk>); they are only compared for equality, any
 * int32 is an id.
 *
 * Alignment of a pair (a = hypothesis, b = reference): matches at cost 0; substitutions, insertions (a word of a left
 * unmatched) and deletions (a word of b left unmatched) at cost 1 each.  cost is the minimum total; among the minimum-cost
 * alignments the one with the FEWEST INSERTIONS is reported.  ins - del = len(a) - len(b) holds for every alignment, so that
 * one also has the fewest deletions and the most substitutions, and one integer fixes the breakdown; the rule is symmetric:
 * (b, a) gives the same cost and sub with ins and del exchanged.  Integer arithmetic, exact.
 * Lengths run from 0 to BLM_EDIT_MAX_LEN.  A BAD pair gets -1 in every output and reads nothing out of range: a sequence
 * index outside [0, n_seq), an offset range that is reversed or leaves [0, n_tok], a length over the limit.  (off, a and b
 * live on the device: this is the kernel's check, not the host's.)
 * cost: (P) int32; sid: (P, 3) int32 sub / ins / del, may be NULL.  Two kernel forms share a call, each taking its own pairs:
 * a lane per pair where the shorter sequence has at most "edit_lane_max" words (option, 0..32, default 32), a wave per pair
 * on a blocked anti-diagonal otherwise; both give the same integers.  No atomics, no workspace.
 * BLM_ERR_INVALID, before any launch: NULL off, a, b or cost, NULL tok with n_tok > 0, a negative count, extents too large
 * (n_tok, n_seq, P at most 2^30).  P == 0: BLM_OK, nothing launched.
 * -------------------------------------------------------------------------- */
#define BLM_EDIT_MAX_LEN 1023
int blm_edit_distance(const int32_t* tok, int64_t n_tok, const int64_t* off, int n_seq, const int32_t* a, const int32_t* b, int P,
                      int32_t* cost, int32_t* sid, void* stream);
/* Selection.  Utterance u owns hypotheses uoff[u] .. uoff[u + 1] (U + 1 int64 offsets on the device; a reversed range is an
 * empty group).  Each hypothesis has, in float64 and all as COSTS (lower is better): the acoustic cost ac, the graph cost g
 * (lmwt.nolm), the old LM's cost lm (lmwt.lmonly), the neural cost nn (what the scorer writes) and the word count len.  Each of
 * the five arrays may be NULL and then counts as zeros.  A grid point is (L, w, p, s): the LM weight L, finite and > 0; the
 * nnweight w; the word insertion penalty p; the posterior scale s, finite and >= 0 (blm_nbest_mbr alone reads it).
 *   T = ac + L * (((g + w * nn) + (1 - w) * lm) + p * len)
 * evaluated in float64 exactly as written, without contraction: stage 7's sum, ranked as Kaldi ranks it at
 * --inv-acoustic-scale=L, multiplied through by L so that no division enters.
 * pick (G, U) int32, grid point k's choice for utterance u at [k * U + u], an index WITHIN the group: the argmin of T with the
 * lowest index on ties; a non-finite T never wins; if every T is non-finite the pick is 0; an empty group gives -1.
 * The grid travels in this host struct, read and validated before the launch and handed to the kernel by value. */
#define BLM_NBEST_GRID_MAX 64
typedef struct blm_nbest_grid {
  uint32_t abi_version; /* BLM_ABI_VERSION */
  int32_t G;            /* 1 .. BLM_NBEST_GRID_MAX points; the entries from G on are not read */
  double lmwt[BLM_NBEST_GRID_MAX];     /* L: finite, > 0 */
  double nnweight[BLM_NBEST_GRID_MAX]; /* w */
  double wip[BLM_NBEST_GRID_MAX];      /* p */
  double pscale[BLM_NBEST_GRID_MAX];   /* s: finite, >= 0 */
} blm_nbest_grid;
/* One workgroup per utterance, lanes over hypotheses, grid points in a loop; (T, index) reduced in a fixed order.
 * BLM_ERR_INVALID, before any launch: NULL uoff, grid or pick, U < 0, G outside 1..BLM_NBEST_GRID_MAX, an L that is not finite
 * or not > 0, an s that is negative or not finite, extents too large; BLM_ERR_ABI: abi_version.  U == 0: BLM_OK. */
int blm_nbest_select(const double* ac, const double* g, const double* lm, const double* nn, const double* len, const int64_t* uoff,
                     int U, const blm_nbest_grid* grid, int32_t* pick, void* stream);
/* Minimum Bayes risk.  With T as above over the group's N hypotheses, H hypotheses in all (uoff must stay inside [0, H]: a range
 * that does not is an empty group):
 *   P_i = exp(-(s * (T_i - min T) / L)) / sum_j of the same;   R_i = sum_j P_j d(i, j), j ascending, in float64
 * and the pick is the argmin of R with the lowest index on ties (-1 for an empty group).  A non-finite T has P = 0; if no T is
 * finite the posterior is uniform.  d is the utterance's dense N x N int32 distance block at dist + doff[u] (doff: U int64 on
 * the device), SYMMETRIC as a distance is: the kernel reads element (j, i) for d(i, j), the order in which neighbouring lanes
 * read neighbouring words.  One workgroup per (utterance, grid point); P is formed in LDS (once when N <= 2048, else chunk by
 * chunk); each lane sums its own rows; no atomics: the same bits in every run.
 * risk: (G, H) float64, R of hypothesis h at grid point k at [k * H + h], may be NULL.  pick as blm_nbest_select's.
 * BLM_ERR_INVALID: as blm_nbest_select, and NULL dist or doff, H < 0. */
int blm_nbest_mbr(const double* ac, const double* g, const double* lm, const double* nn, const double* len, const int64_t* uoff,
                  int U, int64_t H, const int32_t* dist, const int64_t* doff, const blm_nbest_grid* grid, double* risk, int32_t* pick,
                  void* stream);

/* --------------------------------------------------------------------------
 * Search on the incremental path (csrc/beam.hip): the k best next words, beam selection, top-k / nucleus sampling.
 *
 * One total order of a row's entries is used throughout: value descending, then index ascending; -0 equals +0 and every NaN
 * ranks below -inf (a stream that took no token has an all-NaN row).  Values are copied, never recomputed, and the selection
 * uses integer atomics only: results are exact and the same in every run, deterministic mode or not.
 * ------------------------------------------------------------------------ */
#define BLM_TOPK_MAX 256
/* vals / ids (R, k) contiguous: the k first entries of x[r, :V] (row stride ldx >= V) in the order above, best first.
 * 1 <= k <= min(V, BLM_TOPK_MAX).  No workspace. */
int blm_topk_rows(const float* x, int64_t ldx, int R, int V, int k, float* vals, int64_t* ids, void* stream);
/* One beam-search step for G groups of B beams (stream g * B + b), one workgroup per group.  cand_vals / cand_ids (G * B, k):
 * the candidates of every beam (blm_topk_rows of its next-word log-probabilities); score / finished (G * B,): the state before
 * the step.  A live beam b offers (score[b] + cand_vals[b, j], token cand_ids[b, j]) -- one fp32 add each; a finished beam
 * offers itself alone (score unchanged, token eos).  The new beams of a group are its B best candidates by score descending
 * (NaN last), then flat candidate index b_local * k + j ascending.  parent is the GLOBAL stream index of the beam continued
 * (always inside the group); finished_out = parent finished or token == eos.  1 <= B <= BLM_TOPK_MAX, k >= 1; with k >= B the
 * result is the exact top B of all B x V continuations.  score_out / finished_out must not alias score / finished.
 * Start a search from scores [0, -inf, ..., -inf] per group, or the first step picks B copies of one word. */
int blm_beam_select(const float* cand_vals, const int64_t* cand_ids, const float* score, const uint8_t* finished, int G, int B, int k,
                    int64_t eos, float* score_out, uint8_t* finished_out, int64_t* parent, int64_t* token, void* stream);
/* The finished-hypothesis pool of blm_beam_select_pool: P slots for each of G groups, all caller-owned device memory.  Slots
 * [0, count[g]) of group g are its entries in POOL ORDER, best first: norm descending (NaN last, -0 == +0), then insertion
 * order ascending.  The entry point never touches a slot at or past count[g].  Start a search from count = inserted = 0. */
typedef struct blm_beam_pool {
  uint32_t abi_version; /* BLM_ABI_VERSION */
  int32_t P;            /* slots per group, 1 <= P <= BLM_TOPK_MAX */
  float* norm;          /* (G, P) raw * inv_norm of the step that pooled the entry: what the pool is ranked by */
  float* raw;           /* (G, P) cumulative log-probability, the closing eos included */
  int32_t* len;         /* (G, P) length in words, the closing eos included */
  int32_t* step;        /* (G, P) the `step` argument of the call that pooled the entry */
  int64_t* parent;      /* (G, P) GLOBAL stream index: of the beam BEFORE that step which the eos ended (finished = 1); of
                         * the beam AFTER that step, i.e. the slot of that call's parent / token outputs (finished = 0) */
  uint8_t* finished;    /* (G, P) 1: ended by eos; 0: cut off alive by a flush step */
  int32_t* count;       /* (G,) entries held, <= P */
  int64_t* inserted;    /* (G,) entries ever offered to the pool, kept or not */
} blm_beam_pool;
/* One step of a beam search that moves ended hypotheses to a pool and refills the beam, for G groups of B beams (stream
 * g * B + b), one workgroup per group.  cand_vals / cand_ids (G * B, k) as for blm_beam_select, the ids of one beam distinct
 * (blm_topk_rows' are); score (G * B,) raw cumulative log-probability and live (G * B,) before the step.  Scalars: `len`, the
 * length in words of a hypothesis that ends at this step (its eos counted); `step`, stored with what is pooled; `min_len`;
 * inv_norm = float32(1 / len ** a) and inv_norm_max = float32(1 / Lmax ** a), formed by the caller in float64 and rounded once
 * (a >= 0 the length penalty, Lmax the greatest length the search can reach): 0 <= inv_norm_max <= inv_norm < inf.
 *   Candidates.  A live beam b offers (s = score[b] + cand_vals[b, j], token cand_ids[b, j]) for j < k -- one fp32 add each.
 *     A dead beam offers nothing; a candidate whose s is NaN or -inf is no candidate; nor is an eos candidate when
 *     len < min_len.
 *   Order.  s descending, then flat index b_local * k + j ascending.
 *   Walk, over ranks 0 .. min(2 B, B k) - 1 of that order (rank from 0, eos candidates counted):  an eos candidate of rank < B
 *     is OFFERED to the pool as (norm = s * inv_norm -- one fp32 multiply --, raw = s, len, step, parent = g * B + b,
 *     finished = 1); an eos candidate of rank >= B is discarded; the first B candidates that are not eos become the new beams
 *     0, 1, ... in walk order: score_out = s, live_out = 1, parent = g * B + b, token.  A beam has at most one eos candidate,
 *     so with k >= min(2 B, V) these ranks hold everything the exact search over all B x V continuations would reach.  With
 *     fewer than B such candidates the remaining beams are dead: score_out = -inf, live_out = 0, parent = the beam's own
 *     stream index, token = eos.
 *   Flush (flush != 0, the last step).  After the walk every new live beam, in beam order, is offered as (norm = s * inv_norm,
 *     raw = s, len, step, parent = its own NEW stream index, finished = 0).
 *   Pool.  Entries are offered one after the other -- the eos candidates in walk order, then the flushed beams --, each
 *     raising inserted[g] by one.  While count[g] < P an offered entry is inserted at its place in pool order.  Once the pool
 *     is full it replaces the LAST entry only if it precedes it, i.e. if its norm is strictly greater (or the last norm is NaN
 *     and its own is not): it is later in insertion order than everything the pool holds.
 *   Stopping.  Log-probabilities are <= 0 and a >= 0, so no continuation of a beam of score r can be pooled with a norm above
 *     r * inv_norm_max (the same fp32 multiply).  done_out[g] = 1 when, after the step, no beam of the group is live -- after a
 *     flush none is -- or the pool is full and its last norm is STRICTLY greater than that bound for new beam 0, the group's
 *     best (a tie does not stop the group).  The beams of a done group are written dead: score_out = -inf, live_out = 0, parent
 *     and token as the walk left them.  It then offers nothing, so its pool stays as it is, and it is done again, in every
 *     later call.  *all_done = 1 when every group is done, else 0 (written by a second, one-workgroup launch).
 * 1 <= B, 2 B <= BLM_TOPK_MAX, k >= min(2 B, V), len >= 1, step >= 0, min_len >= 0.  score_out / live_out must not alias score /
 * live; float and int32 operands 4-byte, int64 operands 8-byte aligned.  Integer atomics in LDS only, no floating-point
 * atomics and no value recomputed: the result is exact and does not depend on the order in which waves run. */
int blm_beam_select_pool(const float* cand_vals, const int64_t* cand_ids, const float* score, const uint8_t* live, int G, int B, int k,
                         int V, int64_t eos, int step, int len, int min_len, float inv_norm, float inv_norm_max, int flush,
                         const blm_beam_pool* pool, float* score_out, uint8_t* live_out, int64_t* parent, int64_t* token,
                         uint8_t* done_out, uint8_t* all_done, void* stream);
/* blm_sample_rows restricted to an allowed set: with q = softmax(x / temperature), the first top_k entries of the order above
 * (0: all; not capped by BLM_TOPK_MAX) intersected with the shortest prefix of that order whose q-mass reaches top_p (in (0, 1];
 * 1: all; never empty).  The draw is the arg-max over the allowed set of x / temperature + the SAME Philox Gumbel noise as
 * blm_sample_rows (same counter and key): top_k = 0, top_p = 1 returns what blm_sample_rows returns.  temperature 0: argmax.
 * The cuts are found by radix selection over the row (entry counts, and for top_p per-bin mass in integer fixed point, so
 * no floating-point sum depends on an order), not by sorting it. */
int blm_sample_rows_filtered(const float* x, int64_t ldx, int R, int V, float temperature, int top_k, float top_p, const blm_rng* rng,
                             int64_t* out, void* stream);
/* Speculative sampling, the verification of G drafted words per stream in one launch (csrc/speculative.hip; Leviathan et al.
 * 2023, Chen et al. 2023; the loop around it is bayeslms_amd/speculative.py).  The Greek letters of the usual statement are
 * spelled out: tau, beta, rho.
 *
 * The target rows are P (G + 1, N, V) with row stride ldp.  The draft rows are Q (G, N, V) with row stride ldq.  Both hold logits
 * or log-probabilities: the kernel normalises, as blm_row_stats does.  The drafted ids are x (G, N) int64.  tau = temperature,
 * and rng is a blm_rng.  Row index r = t * N + n.
 *
 * For tau > 0, with beta = float32(1 / tau):
 *   p = softmax(beta P[t, n]) and q = softmax(beta Q[t, n]) over the first V columns.  A -inf column has mass 0.
 *   Acceptance.
 *     u_r is the blm_sample_rows uniform, ((w >> 8) + 0.5) * 2^-24, of the first Philox word at counter
 *     (0xFFFFFFFF, r, rng->stream, rng->step), key rng->seed.  No vocabulary column can reach that column value.
 *     accept[t, n] = 1 iff log u_r < min(0, log p(x) - log q(x)), both logs formed from max-shifted values.
 *     An x outside [0, V) or with q(x) = 0 is rejected.
 *   Candidate, t < G (the word emitted if t is the first rejected position).
 *     rho_v = max(p_v - q_v, 0).
 *     cand[t, n] = argmax over v with rho_v > 0 of log rho_v + g_v, lowest index on ties.
 *     g_v = -log(-log u) is blm_sample_rows' Gumbel noise at counter (v, r, rng->stream, rng->step), first word.
 *     If no column has rho_v > 0, the candidate is the plain draw of the next item applied to p.
 *   Candidate, t = G (the bonus word when every draft was accepted).
 *     cand[G, n] = argmax_v beta P_v + g_v.  This is exactly what blm_sample_rows returns for that row of P at that row index
 *     with the same rng.  This is tested bit for bit.
 *   Finish.
 *     n_acc[n] = the smallest t with accept[t, n] = 0, or G if there is none.
 *     token[n] = cand[n_acc[n], n].
 *
 * For tau = 0 (greedy):
 *   Q may be NULL.
 *   accept[t, n] = 1 iff x equals the lowest index holding the maximum of P[t, n].
 *   cand[t, n] is that index, for every t <= G.
 *
 * A row of P or Q (tau > 0) that holds a NaN gives accept = 0 and cand = -1 in that row only.
 *
 * INDEPENDENCE IS THE CALLER'S JOB: the (stream, step) of this call must differ from the ones under which the x were drawn.
 * Otherwise the residual draw reuses the draft's noise and the output is no longer the target's distribution.
 *
 * One workgroup per row (t, n), whether or not an earlier position of the stream rejected; a second small launch walks every
 * stream's G flags.  No atomics, every reduction in a fixed order: the same bits from every run.  No workspace.  Refused with
 * BLM_ERR_INVALID before any launch: a NULL pointer (q may be NULL at tau = 0 only; rng may be NULL there too), G < 1, N < 1,
 * V <= 0, ldp < V or ldq < V, a tau that is negative or not finite or whose 1 / tau is no finite float32, extents beyond
 * 2^30 each / 2^40 elements together, and outputs that overlap the inputs. */
int blm_spec_accept(const float* p, int64_t ldp, const float* q, int64_t ldq, const int64_t* draft, int G, int N, int V,
                    float temperature, const blm_rng* rng, uint8_t* accept /* (G, N) */, int64_t* cand /* (G + 1, N) */,
                    int32_t* n_acc /* (N) */, int64_t* token /* (N) */, void* stream);

/* Cross entropy over materialised logits (M, V) (train.py:233,332;
 * compute_sentence_scores_bayes_jianwei.py:168):
 *   nll[m] = logsumexp(logits[m,:]) - logits[m,tgt[m]]
 * lse (optional) receives logsumexp per row.  If dlogits != NULL also writes (in place allowed) the gradient of
 * mean-NLL: (softmax - onehot) * grad_scale.  loss_sum (+=) sum of nll. */
int blm_ce_fwd_bwd(const float* logits, int64_t ld, const int64_t* tgt, float* nll, float* lse, float* loss_sum,
                   float* dlogits, float grad_scale, int M, int V, void* stream);
/* Deferred gradient: dlogits = (exp(logits - lse[m]) - onehot) * g_dev[0] * scale
 * (in place allowed), for callers that do not know the upstream gradient at
 * forward time. */
int blm_ce_bwd(const float* logits, int64_t ld, const int64_t* tgt, const float* lse, const float* g_dev, float scale,
               float* dlogits, int M, int V, void* stream);

/* Scoring with two interpolated models (compute_sentence_scores_bayes_jianwei.py:157-168: the
 * LOGITS are mixed, alpha*a + (1-alpha)*b, before the log-softmax): per-row NLL in one pass over
 * both logit matrices (M, V), the mixture is never stored.  Forward only. */
int blm_ce_interp_fwd(const float* logits_a, const float* logits_b, int64_t ld, float alpha, const int64_t* tgt,
                      float* nll, int M, int V, void* stream);

/* Distillation loss (engine only: the reference trains on hard labels alone and has no counterpart): cross entropy of
 * softmax(logits) against a DENSE target distribution q = exp(logq) -- a teacher's log-probabilities, e.g. the log pbar of
 * blm_linear_mc_logprobs ("Bayesian dark knowledge": the student learns the posterior predictive) -- interpolated with the
 * hard-label cross entropy, and its gradient, in one pass.  logits (M, V) row stride ld, logq (M, V) row stride ldq; an entry
 * of logq may be -inf (q = 0).  Per row, with z = logits[m,:], l = logq[m,:], Q = sum_v q_v (carried, not assumed 1: a teacher
 * row with masked columns stays exact), lse = logsumexp_v z_v, p_v = exp(z_v - lse), t = tgt[m], valid = 0 <= t < V:
 *   nll[m]  = valid ? lse - z_t : 0                          (as blm_ce_fwd_bwd)
 *   soft[m] = Q lse - sum_{q_v > 0} q_v z_v                   (cross entropy of p under q)
 *   kl[m]   = sum_{q_v > 0} q_v (l_v - z_v + lse)             (KL(q || p) for Q = 1; summed term by term, never as soft - H[q])
 *   loss[m] = (1 - lambda) nll[m] + lambda soft[m]
 *   dlogits[m,v] = ((1 - lambda) valid (p_v - [v = t]) + lambda (Q p_v - q_v)) grad_scale
 * which is the gradient of grad_scale * sum_m loss[m]; a row without a valid hard target still gets its soft part.
 * loss (M) is required; nll, soft, kl, lse (M each) are optional; loss_sum (optional) += sum_m loss[m], added in a fixed order;
 * dlogits (optional, row stride ld) may be logits itself (in place).  BLM_ERR_INVALID, before any launch: a NULL required
 * pointer, ld < V or ldq < V, M < 0 or V <= 0, lambda outside [0, 1] or NaN, dlogits overlapping logq, or overlapping logits
 * other than exactly in place.  M == 0 is a no-op.  One workgroup per row: for V <= 36864 with both strides multiples of 4 and
 * 16-byte aligned bases both rows are held in registers and each is read from memory once; otherwise a guarded two-sweep
 * form.  No floating-point atomics: every run gives the same bits. */
int blm_ce_soft_fwd_bwd(const float* logits, int64_t ld, const float* logq, int64_t ldq, const int64_t* tgt, float lambda,
                        float* loss, float* nll, float* soft, float* kl, float* lse, float* loss_sum, float* dlogits,
                        float grad_scale, int M, int V, void* stream);
/* The same loss against TOP-K teacher targets: the dense logq, ldq of blm_ce_soft_fwd_bwd replaced by a sparse row per token,
 * ids (M, K) int32 and logq (M, K) float32, both with row stride ldk >= K (in elements), 1 <= K <= BLM_TOPK_MAX; every other
 * argument as there and in the same order.  Per row m, with z, lse, p, t, valid as above:
 *   entry j is LIVE when 0 <= ids[m,j] < V; any other id marks an empty slot (-1 by convention) whose logq is never read
 *   q_j = exp(logq[m,j]) (-inf: q_j = 0),  Q = sum_{j live} q_j   (carried, not assumed 1: the K best entries of a teacher
 *                                                                   hold less than all of its mass)
 *   nll[m]  = valid ? lse - z_t : 0
 *   soft[m] = Q lse - sum_{q_j > 0} q_j z[ids_j]
 *   kl[m]   = sum_{q_j > 0} q_j (logq_j - z[ids_j] + lse)           (summed term by term)
 *   loss[m] = (1 - lambda) nll[m] + lambda soft[m]
 *   dlogits[m,v] = ((1 - lambda) valid (p_v - [v = t]) + lambda (Q p_v - sum_{j live, ids_j = v} q_j)) grad_scale
 * On a dense teacher that is -inf outside the live ids this is blm_ce_soft_fwd_bwd.  The live ids of one row must be distinct
 * (blm_topk_rows' are); with duplicates the values at that column are unspecified, and nothing is read or written out of
 * bounds.  loss is required; nll, soft, kl, lse are optional; loss_sum (optional) += sum_m loss[m], added in a fixed order;
 * dlogits (optional, row stride ld) may be logits itself (in place).  BLM_ERR_INVALID, before any launch: NULL logits, ids, logq,
 * tgt or loss, M < 0 or V <= 0, K < 1 or K > BLM_TOPK_MAX, ld < V or ldk < K (or M x stride not an addressable extent), lambda
 * outside [0, 1] or NaN, dlogits overlapping ids or logq, or overlapping logits other than exactly in place.  M == 0 is a no-op.
 * One workgroup per row; the logit row is read from memory once, the 2 K teacher values once: for 4 <= V <= 65536 with ld a
 * multiple of 4 and 16-byte aligned logits / dlogits the row is held in registers, otherwise a guarded two-sweep form; ids and
 * logq rows need no alignment beyond their element type.  No floating-point atomics: every run gives the same bits. */
int blm_ce_soft_topk_fwd_bwd(const float* logits, int64_t ld, const int32_t* ids, const float* logq, int64_t ldk, int K,
                             const int64_t* tgt, float lambda, float* loss, float* nll, float* soft, float* kl, float* lse,
                             float* loss_sum, float* dlogits, float grad_scale, int M, int V, void* stream);
/* The distillation loss with a softmax TEMPERATURE T on its soft term (Hinton et al. 2015): the hard-label term stays at
 * temperature 1, the soft term compares softmax(z / T) with the teacher -- or the model average -- raised to 1 / T and
 * renormalised.  Arguments as blm_ce_soft_fwd_bwd, with beta and soft_scale behind lambda.
 * beta = 1/T > 0.  c = soft_scale >= 0.  z is a row of student logits.  t is the hard target.  valid = 0 <= t < V.
 * Dense teacher row l (log-probabilities, defined up to a constant; -inf means a zero of the teacher):
 *   live_v = l_v > -inf.   has_q = any live.   ml = max over live l_v.
 *   e_v = exp(beta (l_v - ml)), and 0 where not live.   Z = sum e_v.
 *   q~_v = e_v / Z.  This is the teacher (or model average) raised to beta and renormalised over its live entries: pbar^beta / Z.
 *   m = max z.
 *   lse = m + log sum exp(z_v - m).   p_v = exp((z_v - m) - log sum exp(z - m)).
 *   s_beta = sum exp(beta (z_v - m)).   lse_beta = beta m + log s_beta.   p~_v = exp(beta (z_v - m) - log s_beta).
 *   Both p and p~ are formed from the max-shifted logits, never as exp(beta z - lse_beta).
 *   nll[m]  = valid ? lse - z_t : 0.
 *   soft[m] = has_q ? lse_beta - beta sum_live q~_v z_v : 0.  This is the cross entropy of p~ under q~, unscaled.
 *   kl[m]   = sum_live q~_v ((beta (l_v - ml) - log Z) - (beta (z_v - m) - log s_beta)).  It is summed term by term and is >= 0
 *             up to rounding.
 *   loss[m] = (1 - lambda) nll + lambda c soft.
 *   dlogits[m,v] = ((1 - lambda) valid (p_v - [v = t]) + lambda c beta has_q (p~_v - q~_v)) grad_scale.  This is the gradient of
 *             grad_scale * sum_m loss[m].
 *   lse output: the temperature-1 lse, as blm_ce_soft_fwd_bwd's.
 * The tempered target is always normalised (sum q~ = 1).  The untempered kernels carry Q = sum q as it is.  So at beta = 1, c = 1
 * the two agree for a teacher row with Q = 1 and differ by the factor Q otherwise.  c = T^2 is Hinton's scaling: the soft
 * gradient is then lambda T (p~ - q~), and its size does not fall as 1/T when T grows.
 * BLM_ERR_INVALID, before any launch: everything blm_ce_soft_fwd_bwd refuses; a beta that is not finite or not > 0; a soft_scale
 * that is negative or not finite.  The kernel forms, their conditions, the in-place gradient, loss_sum and the fixed order of
 * every sum (no floating-point atomics: the same bits from every run) are blm_ce_soft_fwd_bwd's; the two-sweep form makes a
 * third sweep here (maxima, sums, gradient). */
int blm_ce_soft_temp_fwd_bwd(const float* logits, int64_t ld, const float* logq, int64_t ldq, const int64_t* tgt, float lambda,
                             float beta, float soft_scale, float* loss, float* nll, float* soft, float* kl, float* lse,
                             float* loss_sum, float* dlogits, float grad_scale, int M, int V, void* stream);
/* ... against TOP-K teacher targets: arguments as blm_ce_soft_topk_fwd_bwd, with beta and soft_scale behind lambda.  Sparse
 * (top-k) teacher row: the same definitions hold with "live" meaning 0 <= ids_j < V and logq_j > -inf, and z_v read at ids_j; a
 * column that no live entry names has q~ = 0.  A constant added to a row's logq cancels in q~.  So targets stored renormalised
 * or not give the same tempered loss, and one file of cached top-k targets serves every temperature.  On a dense teacher
 * that is -inf outside the live ids this is blm_ce_soft_temp_fwd_bwd.  Refuses what blm_ce_soft_topk_fwd_bwd refuses, and beta /
 * soft_scale as above; duplicate live ids as there. */
int blm_ce_soft_topk_temp_fwd_bwd(const float* logits, int64_t ld, const int32_t* ids, const float* logq, int64_t ldk, int K,
                                  const int64_t* tgt, float lambda, float beta, float soft_scale, float* loss, float* nll,
                                  float* soft, float* kl, float* lse, float* loss_sum, float* dlogits, float grad_scale, int M,
                                  int V, void* stream);


/* dcoef[i,n] += sum_m g[m,n] * act_i(z[m,n]), i = tanh, sigmoid, relu, gelu: gradient of the GPNN
 * mixture coefficients (autograd of model.py:1885-1899). */
int blm_gp_coef_grad(const float* g, const float* z, float* dcoef, int M, int N, void* stream);

/* out[n] (+)= sum_m x[m,n]   (bias gradients). */
int blm_colsum(const float* x, int64_t ld, float* out, int M, int N, int accumulate, void* stream);
/* ... and the same sums into a second vector out2 (NULL: none) from the same pass: nn.LSTM's b_ih and b_hh receive the same
 * gradient (model.py:35 / _VF.lstm :812).  For callers that bind the ABI directly: the Python host of this repository takes the
 * bias gradients out of the weight-gradient GEMM (blm_gemm_args.colsum_a) and adds them to both leaves with blm_init_multi, so
 * nothing under bayeslms_amd/ calls this entry point (it is covered at kernel level, tests/test_gpu_kernels.py and
 * tests/test_gpu_update_kernels.py).  With accumulate == 0 out2 is a copy of out, bit for bit; with accumulate != 0 each vector
 * takes the row chunks' float atomics in an order of its own.  In deterministic mode (blm_set_option("deterministic", 1)) both
 * column-sum entry points use one row chunk: one writer per sum, and two vectors that start equal stay equal. */
int blm_colsum2(const float* x, int64_t ld, float* out, float* out2, int M, int N, int accumulate, void* stream);
/* Up to 8 small vectors set by ONE launch: dst[i][0..n[i]) = (src[i] ? src[i][j] : 0) + (src2[i] ? src2[i][j] : 0); src / src2
 * may be NULL altogether.  dst, src, src2, n are HOST arrays (copied into the launch).  The set-up of a recurrent layer -- initial
 * states into row 0 of the state histories, b_ih + b_hh, zeroed gradient carries -- is 8-12 launches of ~5 us without it. */
int blm_init_multi(int count, float* const* dst, const float* const* src, const float* const* src2, const int64_t* n,
                   void* stream);

/* Global-norm clip + SGD momentum over a list of tensors (train.py:419-420,466):
 *   norm = sqrt(sum_i |g_i|^2); c = min(1, clip/(norm+1e-6));
 *   buf = first ? c*g : mom*buf + c*g;  p -= lr*buf
 * Two calls: blm_sqnorm_multi adds the squared norm to *sq (zeroed by the
 * caller) through per-block partials in ws (>= blm_sqnorm_ws_floats(n)) summed
 * in a fixed order -- deterministic, so data-parallel replicas stay bit-identical;
 * blm_clip_sgd_multi consumes it.  Pointer tables are DEVICE arrays of n
 * pointers/sizes. */
int64_t blm_sqnorm_ws_floats(int n);
int blm_sqnorm_multi(const float* const* grads, const int64_t* sizes, int n, float* sq, float* ws, void* stream);
int blm_clip_sgd_multi(float* const* params, const float* const* grads, float* const* bufs, const int64_t* sizes,
                       int n, const float* sq, float clip, float lr, float momentum, int first, float grad_scale,
                       void* stream);

/* One whole LSTM time step in a single launch (recurrent product on the matrix
 * cores + the cell below fused behind it; model.py:812 `_VF.lstm` per step):
 *   gates = xw_t[b,4H] + h_prev[b,H] . w_hh[4H,H]^T ; then the cell update;
 *   h_noise (H floats, may be NULL) is added to every row of h afterwards (the Variational
 *   LSTM's h += eps*exp(hidden_lgstd), model.py:2523-2527).
 * Requires H % 32 == 0 and 16-byte aligned h_prev / w_hh; otherwise returns
 * BLM_ERR_UNSUPPORTED and the caller composes blm_gemm + blm_lstm_cell_fwd.
 * Deterministic (fixed summation order, no atomics). */
int blm_lstm_step_fwd(const float* xw_t, const float* w_hh, const float* h_prev, const float* c_prev, float* h,
                      float* c, float* gates_act, const float* h_noise, int B, int H, void* stream);

/* The T forward steps of one layer from ONE call (T launches of blm_lstm_step_fwd issued by the library: a scoring
 * pass has nothing to hide the caller's per-call cost behind).  xw (T,B,4H); hs, cs (T+1,B,H) with row 0 = the
 * initial state, rows 1..T written; gates_act (T,B,4H) or NULL; noise_rows (T,H) or NULL.  Same shape rule and
 * status codes as blm_lstm_step_fwd (nothing is launched when the first step is unsupported). */
int blm_lstm_seq_fwd(const float* xw, const float* w_hh, float* hs, float* cs, float* gates_act, const float* noise_rows,
                     int T, int B, int H, void* stream);
/* Two independent recurrences side by side: step t of sequence A (n_a steps) and step t of sequence B (n_b steps) per launch for
 * B <= 4 (the scorer's B = 1 carry chain: layer 1 over chunk c beside layer 2 over chunk c - 1 -- one launch per step pair
 * instead of two; larger batches and the unpaired remainder run as blm_lstm_step_fwd launches).  Buffers as blm_lstm_seq_fwd,
 * per sequence; n_a or n_b may be 0. */
int blm_lstm_seq_pair_fwd(const float* xw_a, const float* w_hh_a, float* hs_a, float* cs_a, float* ga_a, int n_a,
                          const float* xw_b, const float* w_hh_b, float* hs_b, float* cs_b, float* ga_b, int n_b,
                          int B, int H, void* stream);

/* Backward of one LSTM time step in a single launch:
 *   dh = dgates_t[b,4H] . w_hh[4H,H]   (w_hh passed TRANSPOSED: w_hh_t (H,4H), see blm_transpose)
 * then, when dgates_out != NULL, the cell backward of the previous step (blm_lstm_cell_bwd2 with
 * dh = this product, dh2 = dy_prev): dgates_out (B,4H) and dc_prev (B,H) are written and dh itself
 * never reaches memory unless dh_out != NULL.  dgates_out == NULL: only dh_out is written.
 * Same shape/alignment rule and status codes as blm_lstm_step_fwd. */
int blm_lstm_step_bwd(const float* dgates_t, const float* w_hh_t, const float* dy_prev, const float* dc_next,
                      const float* c_prev, const float* c, const float* gates_act, float* dgates_out, float* dc_prev,
                      float* dh_out, int B, int H, void* stream);
/* The backward steps t_hi-1 .. t_lo (descending) of one layer from ONE call -- blm_lstm_seq_fwd's counterpart: step T-1 is
 * the plain cell backward (blm_lstm_cell_bwd2 with dh = dh_T, dh2 = dy[T-1]), every earlier step t one blm_lstm_step_bwd
 * launch (dh = dgates[t+1] . w_hh, then the cell of step t).  dy (T,B,H); cs (T+1,B,H) as blm_lstm_seq_fwd leaves them;
 * gates_act, dgates (T,B,4H); dc_pair (2,B,H): slot k holds the dc arriving from above on entry, the slots alternate per
 * step, so the caller's next k is k ^ ((t_hi - t_lo) & 1); dh_rows (T,B,H) or NULL: row t receives the product of step t's
 * launch (what h_t gets from step t+1).  dh_T is read only when t_hi == T.  A chain may be walked in several calls
 * (t_hi of one = t_lo of the one before): the layer wavefront does, chunk by chunk. */
int blm_lstm_seq_bwd(const float* dh_T, const float* dy, const float* cs, const float* gates_act, const float* w_hh_t,
                     float* dgates, float* dc_pair, int k, float* dh_rows, int T, int t_hi, int t_lo, int B, int H,
                     void* stream);
/* The same two step kernels for the GP-LSTM cell with a GPNN on one gate (GPLSTMCell gate types 1-4,
 * model.py:1754-1771): gate `gate_ovr` (0 i, 1 f, 2 g, 3 o; -1 = plain LSTM) takes the activation
 * mixture sum_i act_i(z) coef4[i] of its pre-activation z instead of its sigmoid/tanh.  The caller
 * places the GPNN's weight rows into that gate's row block of w_hh / xw_t.  coef4 is (4,H) in the slot
 * order tanh, sigmoid, relu, gelu.  Forward keeps z (z_out, (B,H)) for the backward pass; backward
 * multiplies that gate's gradient by the mixture's derivative at z_prev and returns the gradient
 * w.r.t. the mixture value in dact_out (B,H) (for blm_gp_coef_grad).
 * gate_ovr = 4 is GPLSTMCell gate type 6 (model.py:1744-1752): the whole hidden projection
 * h_prev . w_hh^T + rbias (4H) passes through the mixture (coef4 (4,4H), z (B,4H)) before it is added
 * to xw_t; backward then also writes dz_out = dgates_out * mixture'(z_prev) (B,4H), which is the
 * dgates_t operand of the next (earlier) step's launch.
 * gate_ovr = 5 is GPLSTMCell gate type 5 (model.py:1759-1760, `cx = self.gpnn(cx)` in front of the cell update): a second
 * recurrent product per step, c_{t-1} . Wg^T.  The caller computes it with blm_lstm_step_dh(c_prev, Wg, z_out, B, H, H)
 * right before this launch; the step kernel adds rbias (H), stores z back into z_out and lets the mixture of z
 * (coef4 (4,H)) take c_prev's place in  c' = f * c_in + i * g.  Backward (gate_ovr = 5, z_prev = that z): the cell
 * backward uses mixture(z_prev) as its incoming cell state, writes dact_out = d c_in (B,H) (for blm_gp_coef_grad) and
 * dz_out = d c_in * mixture'(z_prev) (B,H); the raw cell-state gradient of the earlier step is then
 * blm_lstm_step_dh(dz_out, Wg^T, dc, B, H, H). */
int blm_lstm_step_fwd_gp(const float* xw_t, const float* w_hh, const float* h_prev, const float* c_prev, float* h,
                         float* c, float* gates_act, const float* h_noise, int gate_ovr, const float* coef4,
                         const float* rbias, float* z_out, int B, int H, void* stream);
int blm_lstm_step_bwd_gp(const float* dgates_t, const float* w_hh_t, const float* dy_prev, const float* dc_next,
                         const float* c_prev, const float* c, const float* gates_act, float* dgates_out, float* dc_prev,
                         float* dh_out, int gate_ovr, const float* coef4, const float* z_prev, float* dact_out,
                         float* dz_out, int B, int H, void* stream);
/* out (cols,rows) = in (rows,cols)^T */
int blm_transpose(const float* in, float* out, int rows, int cols, void* stream);

/* LSTM cell pointwise part (what _VF.lstm fuses, model.py:812): gates =
 * xw[b,4H] + hw[b,4H] (biases already inside xw), order i,f,g,o.
 *   c' = sig(f) c + sig(i) tanh(g);  h' = sig(o) tanh(c')
 * Saves activated gates (B,4H) for backward. */
int blm_lstm_cell_fwd(const float* xw, const float* hw, const float* c_prev, float* h, float* c, float* gates_act,
                      int B, int H, void* stream);
/* In: dh (sum of grad from above and from next step), dc_next; out: dgates (B,4H), dc_prev. */
int blm_lstm_cell_bwd(const float* dh, const float* dc_next, const float* c_prev, const float* c, const float* gates_act,
                      float* dgates, float* dc_prev, int B, int H, void* stream);
/* Same with the incoming hidden gradient given as two addends (recurrent part + this step's dy),
 * so the host needs no separate accumulation pass per time step. */
int blm_lstm_cell_bwd2(const float* dh, const float* dh2, const float* dc_next, const float* c_prev, const float* c,
                       const float* gates_act, float* dgates, float* dc_prev, int B, int H, void* stream);
/* GP-LSTM cell (GPLSTMCell.Gplstm, model.py:1745-1777): same cell, but gate `gate_idx` (0 i, 1 f,
 * 2 g, 3 o) takes its ACTIVATED value from gate_ovr (B,H) -- the output of a GPNN -- instead of
 * sigmoid/tanh of its pre-activation.  Backward returns, in slot gate_idx of dgates, the gradient
 * w.r.t. that activated value (d_ovr, (B,H)) and zero pre-activation gradient for it. */
int blm_lstm_cell_ovr_fwd(const float* xw, const float* hw, const float* c_prev, const float* gate_ovr, int gate_idx,
                          float* h, float* c, float* gates_act, int B, int H, void* stream);
int blm_lstm_cell_ovr_bwd(const float* dh, const float* dc_next, const float* c_prev, const float* c,
                          const float* gates_act, int gate_idx, float* dgates, float* d_ovr, float* dc_prev, int B,
                          int H, void* stream);
/* Same with the incoming hidden gradient as two addends (dh2 may be NULL), like blm_lstm_cell_bwd2. */
int blm_lstm_cell_ovr_bwd2(const float* dh, const float* dh2, const float* dc_next, const float* c_prev, const float* c,
                           const float* gates_act, int gate_idx, float* dgates, float* d_ovr, float* dc_prev, int B, int H,
                           void* stream);
/* Elementwise GPNN mixture on pre-activations z (M,N): out = sum_i act_i(z) coef[i,n];
 * backward dz = dout * sum_i act_i'(z) coef[i,n]   (model.py:1885-1899). */
int blm_gp_mix_fwd(const float* z, const float* coef, float* out, int M, int N, void* stream);
int blm_gp_mix_bwd(const float* dout, const float* z, const float* coef, float* dz, int M, int N, void* stream);
/* x[b,:] += v[:]  (VNN hidden-state noise, model.py:2571-2577); rows B, cols H. */
int blm_add_rowvec(float* x, const float* v, int B, int H, void* stream);

/* y (+)= a*x elementwise helpers used by the host glue. */
int blm_axpy(const float* x, float* y, int64_t n, float a, void* stream);
/* dst[v,:] += src[slot[v],:] for every v in [0,V) with 0 <= slot[v] < n_src (rows of D floats).  Data-parallel
 * training reduces the embedding half of the tied encoder/decoder gradient (model.py:1240; the last tensor backward
 * finishes) as a compact matrix of the rows this step touched; this adds it back (engine.LateRows). */
int blm_rows_gather_add(float* dst, const int64_t* slot, const float* src, int64_t V, int D, int64_t n_src, void* stream);

/* --------------------------------------------------------------------------
 * Architecture search (model_search_bayes.py, architect.py,
 * train_search_bayes.py).  HBM-bound streaming kernels.
 * ------------------------------------------------------------------------ */

/* Mix of two candidate branches by the softmax'd architecture weights
 * (model_search_bayes.py:234-236, :77-78):
 *   out = (probs[0]*a + probs[1]*b) * keep        probs: 2 floats on the DEVICE
 * a, b, out are (rows, B, N) activations; dropout (model_search_bayes.py:236
 * `self.dropout(src1)`) as blm_dropout keys it; drop_p == 0 -> none. */
int blm_mix2_fwd(const float* a, const float* b, const float* probs, float* out, int rows, int B, int N, float drop_p,
                 const blm_rng* rng, int col_offset, int global_cols, void* stream);
/* Backward: g = dout*keep; da = probs[0]*g*(mul_a ? mul_a : 1); db = probs[1]*g (either may be NULL);
 * partial[2*j+{0,1}] = block j's share of sum(g*a), sum(g*b) -- blm_mix2_partials(rows,B,N) floats,
 * written (not accumulated), fixed order inside a block; reduce with blm_colsum(partial, 2, dprobs, n/2, 2).
 * mul_a lets the GELU branch fold its derivative (aux of BLM_EPI_BIAS_GELU) into the same pass. */
int64_t blm_mix2_partials(int rows, int B, int N);
int blm_mix2_bwd(const float* dout, const float* a, const float* b, const float* probs, const float* mul_a, float* da,
                 float* db, float* partial, int rows, int B, int N, float drop_p, const blm_rng* rng, int col_offset,
                 int global_cols, void* stream);

/* blm_mix2_bwd for a GP branch b = sum_i act_i(z_b) coef[i] (GaussTransSearchEncoderLayer, model_search_bayes.py:
 * 234-236): dz_b = probs[1]*g*mixture'(z_b) directly (no separate blm_gp_mix_bwd pass over the activations);
 * dhk (may be NULL) = probs[1]*g, the gradient w.r.t. the mixture value that blm_gp_coef_grad needs. */
int blm_mix2_gp_bwd(const float* dout, const float* a, const float* b, const float* probs, const float* mul_a,
                    const float* z_b, const float* coef, float* da, float* dz_b, float* dhk, float* partial, int rows, int B,
                    int N, float drop_p, const blm_rng* rng, int col_offset, int global_cols, void* stream);

/* BayesLSTMSearchCell.bayeslstm pointwise part (model_search_bayes.py:686-710).  z8 = xw8 + hw8 is
 * (B, 8H) with row layout [i f g o | i' f' g' o'] (standard gates, then the four `Bayes` maps);
 * probs (4,2) on the device, rows i,f,g,o:
 *   gate_k = act_k(z_k)*probs[k][0] + act_k(z'_k)*probs[k][1];  c = f*c_prev + i*g;  h = o*tanh(c)
 * acts8 (B,8H, may be NULL) keeps the eight activations for the backward. */
int blm_lstm_search_cell_fwd(const float* xw8, const float* hw8, const float* c_prev, const float* probs, float* h,
                             float* c, float* acts8, int B, int H, void* stream);
/* Backward: dh (+ dh2, may be NULL), dc_next (may be NULL) -> dz8 (B,8H), dc_prev (B,H) and
 * partial[8*j + 2k + s] = block j's share of d probs[k][s]; blm_lstm_search_cell_partials(B,H) floats. */
int64_t blm_lstm_search_cell_partials(int B, int H);
int blm_lstm_search_cell_bwd(const float* dh, const float* dh2, const float* dc_next, const float* c_prev, const float* c,
                             const float* acts8, const float* probs, float* dz8, float* dc_prev, float* partial, int B,
                             int H, void* stream);

/* One whole search-cell time step in a single launch (blm_lstm_step_fwd with eight gate streams):
 *   z8 = xw8_t[b,8H] + h_prev[b,H] . w8_hh[8H,H]^T, then blm_lstm_search_cell_fwd's pointwise part.
 * Same shape rule and status codes as blm_lstm_step_fwd (BLM_ERR_UNSUPPORTED: compose blm_gemm +
 * blm_lstm_search_cell_fwd). */
int blm_lstm_search_step_fwd(const float* xw8_t, const float* w8_hh, const float* h_prev, const float* c_prev,
                             const float* probs, float* h, float* c, float* acts8, int B, int H, void* stream);

/* Backward of one search-cell time step in a single launch (blm_lstm_step_bwd with the search cell fused behind the
 * product): dh = dz8_t (B,8H) . w8_t (H,8H)^T, then blm_lstm_search_cell_bwd of the previous step with dh + dy_prev:
 * dz8_out (B,8H), dc_prev (B,H) and blm_lstm_search_step_partials(B,H) per-block partials of d probs
 * (partial[8*j + 2k + s]); dh never reaches memory.  H % 16 == 0, 16-byte aligned operands. */
int64_t blm_lstm_search_step_partials(int B, int H);
int blm_lstm_search_step_bwd(const float* dz8_t, const float* w8_t, const float* dy_prev, const float* dc_next,
                             const float* c_prev, const float* c, const float* acts8, const float* probs, float* dz8_out,
                             float* dc_prev, float* partial, int B, int H, void* stream);

/* The skinny recurrent dgrad of one search-cell step on the blm_lstm_step_bwd kernel (no cell fused):
 *   dh_out (B,H) = dz (B,G) . w_t (H,G)^T      w_t = the stacked recurrent weight (G,H) TRANSPOSED
 * One launch, fixed summation order, no memset / atomics.  Needs H % 16 == 0, G % 64 == 0, 16-byte
 * aligned operands (BLM_ERR_UNSUPPORTED otherwise: use blm_gemm). */
int blm_lstm_step_dh(const float* dz, const float* w_t, float* dh_out, int B, int H, int G, void* stream);
/* The same product written into a column window of a wider matrix: dh_out has row stride ldo >= H. */
int blm_lstm_step_dh_ld(const float* dz, const float* w_t, float* dh_out, int64_t ldo, int B, int H, int G, void* stream);
/* ... with the GPNN2 activation sum on the way out (feat has row stride ld_f; the product has H output columns):
 *   act_mode 1: the product is the feature matrix f:  feat = f  and  out[:, m] = (f + sum_a a(f)) * scale for m < M,
 *               out[:, M] = 1, 0 for M < m < H                       (blm_gpnn2_actsum_fwd fused behind the product)
 *   act_mode 2: the product is d s:  out[:, m] = d s * (1 + sum_a a'(feat)) * scale for m < M, 0 beyond   (..._bwd) */
int blm_lstm_step_dh_act(const float* dz, const float* w_t, float* out, int64_t ldo, int B, int H, int G, int act_mode, float* feat,
                         int ld_f, int M, float scale, int acts, void* stream);

/* GPNN2 (random-feature GP, model.py:2036-2076) between its two products: features f (rows, ld_f) -> s (rows, ld_s),
 *   s[:, m] = (f + sum_{a in acts} a(f)) * scale   for m < M   (acts: bit set in the slot order 1 tanh, 2 sigmoid, 4 relu,
 *   s[:, M] = 1, zeros beyond                                   8 gelu; model.py:2069-2075 with skip_act)
 * The 1-column lets the caller fold coef.bias into a coefficient matrix padded to ld_s columns.  Backward:
 *   df[:, m] = ds[:, m] * (1 + sum a'(f)) * scale for m < M, 0 on the padding; ds and df have row stride ld_s. */
int blm_gpnn2_actsum_fwd(const float* f, float* s, int64_t rows, int M, int ld_f, int ld_s, float scale, int acts, void* stream);
int blm_gpnn2_actsum_bwd(const float* ds, const float* f, float* df, int64_t rows, int M, int ld_f, int ld_s, float scale,
                         int acts, void* stream);
/* out[r, c] = a[r, c] + b[r, c] for r < rows, c < cols on column windows of wider matrices (row strides lda / ldb / ldo):
 * the pre-activation of ONE gate, xw_t[:, gH:(g+1)H] + (h W_hh^T)[:, gH:(g+1)H], as a contiguous operand. */
int blm_add_cols(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo, int64_t rows, int cols,
                 void* stream);
/* The T frequency matrices of one forward of a GPNN2 that is called at every time step (GPLSTMCell with type digit 4,
 * model.py:1763-1770 -> :2062-2065): F_t = mean + exp(lgstd) * eps_t (H x M), eps_t = eps_all[t] (T,H,M) or the Philox
 * stream (rng0->seed, rng0->stream, rng0->step + t) with blm_sample_weight's element order.  Outputs, zero padded:
 * FT (T, MP, H) = F_t^T and Fp (T, H, GP) = F_t -- the operands of the per-step feature product and of its input gradient. */
int blm_gpnn2_sample_steps(const float* mean, const float* lgstd, const float* eps_all, const blm_rng* rng0, int T, int H, int M,
                           int MP, int GP, float* FT, float* Fp, void* stream);
/* Their gradient in one launch: with G_t = pre_t^T df_t (pre (T,B,H) the GPNN2 inputs, df (T,B,GP) the feature gradients),
 *   dmean += sum_t G_t,   dlgstd += exp(lgstd) * sum_t eps_t * G_t      (either may be NULL). */
int blm_gpnn2_freq_grad(const float* pre, const float* df, const float* eps_all, const blm_rng* rng0, const float* lgstd,
                        float* dmean, float* dlgstd, int T, int B, int H, int M, int GP, void* stream);
/* The time loops of a GP-LSTM layer with a GPNN2 that draws fresh frequencies at every step (GPLSTMCell, type digit 4;
 * model.py:1744-1771), ONE call per direction.  GPNN2_t(x) = (actsum(x F_t) | 1) cwp^T with cwp = [coef.weight | coef.bias | 0]
 * (rows = outputs, GP columns), FT (nF,MP,H) / Fp (nF,H,GP) from blm_gpnn2_sample_steps, nF = T or 1 (mean frequencies).
 *   mode 0  gate types 1-4: z4_t = h_{t-1} w_hh^T; pre_t = xw_t[:, gate] + z4_t[:, gate]; gout_t = GPNN2_t(pre_t) (B,H) is
 *           that gate's activation in the cell update (xw carries both bias_ih)
 *   mode 1  gate type 5:    gout_t = c_in = GPNN2_t(c_{t-1}) (B,H) takes c_{t-1}'s place in the fused step (blm_lstm_step_fwd)
 *   mode 2  gate type 6:    gout_t = GPNN2_t(h_{t-1}) (B,4H; cwp is (4H,GP)) is the hidden projection of all four gates
 * Buffers (T rows each unless noted): hs, cs (T+1,B,H) with row 0 = initial state; ga (B,4H); feat (B,MP); sact (B,GP);
 * mode 0 also z4 (B,4H) and pre (B,H).  Backward walks t = T-1..0: dh (B,H) holds dh_T on entry and dh_0 on exit, dcs2
 * (2,B,H) ping-pongs dc ([0] = dc_T on entry, dc_0 ends in [T & 1]); it fills dgates (T,B,4H) (= d xw; mode 0: the gate's
 * slot holds d pre), df (T,B,GP), da (T,B,H) (modes 0 / 1: the gradient of gout); ds is unused (the activation sum and its
 * derivative ride in the epilogues of the feature / d s products, blm_lstm_step_dh_act; sact's padding columns >= MP must be
 * zero on entry of the forward call); w_hh_t = w_hh^T (H,4H), cwt = cwp^T.  Needs H % 64 == 0, MP % 16 == 0, GP % 64 == 0, M < MP <= GP (BLM_ERR_UNSUPPORTED from the
 * products otherwise). */
typedef struct blm_gpnn2_seq {
  uint32_t abi_version; /* BLM_ABI_VERSION */
  int32_t mode, gate, acts;
  int32_t T, B, H, M, MP, GP, nF;
  const float *xw, *w_hh, *w_hh_t, *FT, *Fp, *cwp, *cwt;
  float *hs, *cs, *ga, *z4, *pre, *feat, *sact, *gout;
  const float* dy;
  float *dh, *dcs2, *dgates, *da, *ds, *df;
} blm_gpnn2_seq;
int blm_lstm_gpnn2_seq_fwd(const blm_gpnn2_seq* q, void* stream);
int blm_lstm_gpnn2_seq_bwd(const blm_gpnn2_seq* q, void* stream);

/* torch.optim.Adam(lr, betas, eps, weight_decay) on one tensor (architect.py:33): g += wd*p;
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr * (m/(1-b1^step)) / (sqrt(v/(1-b2^step)) + eps).
 * step counts from 1. */
int blm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, void* stream);

/* blm_clip_sgd_multi with torch.optim.SGD's weight decay: the clipped gradient becomes
 * c*g + weight_decay*p before the momentum update (train_search_bayes.py:330,391-392). */
int blm_clip_sgd_multi_wd(float* const* params, const float* const* grads, float* const* bufs, const int64_t* sizes, int n,
                          const float* sq, float clip, float lr, float momentum, int first, float grad_scale,
                          float weight_decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BAYESLM_H */
