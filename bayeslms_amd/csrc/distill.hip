// Distillation loss: cross entropy of softmax(logits) against a DENSE target distribution q = exp(logq) (the teacher's
// log pbar, blm_linear_mc_logprobs, or a mean-weight log-softmax), interpolated with the hard-label cross entropy and fused
// with its gradient the way ce_row_kernel (elementwise.hip) fuses the hard-label one.  Per row m, with z = logits[m, :],
// l = logq[m, :] (-inf: q = 0), Q = sum q, lse = logsumexp z, p = exp(z - lse), t = tgt[m], valid = 0 <= t < V:
//   nll  = valid ? lse - z_t : 0
//   soft = Q lse - sum_{q>0} q z
//   kl   = sum_{q>0} q (l - (z - lse))          summed term by term: the terms are small where the student is close
//   loss = (1 - lambda) nll + lambda soft
//   dz_v = ((1 - lambda) valid (p_v - [v = t]) + lambda (Q p_v - q_v)) grad_scale
// One workgroup per row, every sum in a fixed order, no atomics: the same bits from every run.
// blm_ce_soft_topk_fwd_bwd (below): the same loss against a SPARSE teacher row, the K best entries per token.
// blm_ce_soft_temp_fwd_bwd / blm_ce_soft_topk_temp_fwd_bwd (further below): both with a softmax temperature on the soft term, in
// kernels of their own; the kernels up to there are what temperature 1 runs and are not touched by them.
#include <cmath>
#include <type_traits>

#include "blm_device.h"
#include "blm_host.h"

namespace blm {

struct SoftCoef {
  float p, q, t;  // gradient = p * softmax - q * teacher - t * onehot
};
__device__ __forceinline__ SoftCoef soft_coef(float lambda, bool valid, float Q, float gscale) {
  const float hard = valid ? (1.f - lambda) * gscale : 0.f;
  return {hard + lambda * Q * gscale, lambda * gscale, hard};
}

// one element of the second sweep: its KL term (returned) and its gradient (g)
__device__ __forceinline__ float soft_elem(float z, float l, float lse, const SoftCoef& c, float& g) {
  const float lp = z - lse, q = __expf(l);
  g = c.p * __expf(lp) - c.q * q;
  return q > 0.f ? q * (l - lp) : 0.f;
}

// Both rows held in registers: 1024 threads x NV float4 of each cover V <= 4096 NV, so the logits and the teacher row are
// each read from HBM exactly once, all 2 NV loads of a thread in flight together; Q and sum q z need no lse and are formed
// from the loaded values, the gradient is written from registers (in place over the logits when dlogits == logits).
// Requires ld, ldq multiples of 4 and 16-byte aligned bases (blm_ce_soft_fwd_bwd selects).  logits / dlogits may alias:
// not __restrict__.
template <int NV>
__global__ __launch_bounds__(1024) void ce_soft_row_kernel(const float* logits, long ld, const float* __restrict__ logq, long ldq,
                                                           const int64_t* __restrict__ tgt, float lambda, float* __restrict__ loss,
                                                           float* __restrict__ nll, float* __restrict__ soft,
                                                           float* __restrict__ kl, float* __restrict__ lse_out, float* dlogits,
                                                           float gscale, int V) {
  __shared__ float red[3][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  const float* y = logq + row * ldq;
  const unsigned t0 = threadIdx.x * 4u, Vu = (unsigned)V;  // unsigned: base + 32-bit offset addressing, no 64-bit address per load
  // The registers hold the quads that lie wholly inside the row: one compare per quad, float4 loads and stores only, all 2 NV
  // loads issued back to back (a quad outside reads quad 0 instead -- V >= 4 here -- and is skipped wherever the quads are
  // used).  The V % 4 columns behind the last whole quad are one extra (z, l) pair in threads 0 .. V % 4 - 1.
  float4 v[NV], u[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const unsigned j = t0 + 4096u * i;
    const bool in = j + 3 < Vu;
    const unsigned js = in ? j : 0u;
    v[i] = *reinterpret_cast<const float4*>(x + js);
    u[i] = *reinterpret_cast<const float4*>(y + js);
  }
  const unsigned je = (Vu & ~3u) + threadIdx.x;  // this thread's column behind the whole quads, if je < V
  const bool extra = je < Vu;
  const float ze = extra ? x[je] : -INFINITY, le = extra ? y[je] : -INFINITY;
  const long t = tgt[row];
  const bool valid = t >= 0 && t < V;
  const float xt = valid ? x[t] : 0.f;  // read before any in-place gradient write (the reductions below have barriers)
  const unsigned tu = valid ? (unsigned)t : 0xFFFFFFFFu;  // 32-bit from here on
  const float qe = __expf(le);
  float m = ze, Q = qe, qz = qe > 0.f ? qe * ze : 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;  // tested where the quad is used, behind the loads: none of them waits for another
    m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
    const float q0 = __expf(u[i].x), q1 = __expf(u[i].y), q2 = __expf(u[i].z), q3 = __expf(u[i].w);
    Q += (q0 + q1) + (q2 + q3);
    qz += ((q0 > 0.f ? q0 * v[i].x : 0.f) + (q1 > 0.f ? q1 * v[i].y : 0.f)) +
          ((q2 > 0.f ? q2 * v[i].z : 0.f) + (q3 > 0.f ? q3 * v[i].w : 0.f));
  }
  float M_ = m;
  row_fold<ROW_MAX>(red, M_);
  float l = __expf(ze - M_);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    l += __expf(v[i].x - M_) + __expf(v[i].y - M_) + __expf(v[i].z - M_) + __expf(v[i].w - M_);
  }
  row_fold<ROW_SUM, ROW_EACH>(red, l, Q, qz);
  const float lse = M_ + __logf(l);
  const SoftCoef c = soft_coef(lambda, valid, Q, gscale);
  float* d = dlogits ? dlogits + row * ld : nullptr;
  float ge;
  float k = soft_elem(ze, le, lse, c, ge);
  if (d && extra) d[je] = tu == je ? ge - c.t : ge;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const unsigned j = t0 + 4096u * i;
    if (!(j + 3 < Vu)) continue;
    float4 g;
    k += (soft_elem(v[i].x, u[i].x, lse, c, g.x) + soft_elem(v[i].y, u[i].y, lse, c, g.y)) +
         (soft_elem(v[i].z, u[i].z, lse, c, g.z) + soft_elem(v[i].w, u[i].w, lse, c, g.w));
    if (d) {
      g.x -= tu == j ? c.t : 0.f;
      g.y -= tu == j + 1 ? c.t : 0.f;
      g.z -= tu == j + 2 ? c.t : 0.f;
      g.w -= tu == j + 3 ? c.t : 0.f;
      *reinterpret_cast<float4*>(d + j) = g;
    }
  }
  row_fold<ROW_SUM>(red, k);
  if (threadIdx.x == 0) {
    const float n = valid ? lse - xt : 0.f, s = Q * lse - qz;
    loss[row] = (1.f - lambda) * n + lambda * s;
    if (nll) nll[row] = n;
    if (soft) soft[row] = s;
    if (kl) kl[row] = k;
    if (lse_out) lse_out[row] = lse;
  }
}

// Any V, any stride, any alignment: an online (max, sum exp) sweep that also forms Q and sum q z, then a second sweep over
// both rows (from L2 / the Infinity Cache where they still are) for the KL terms and the gradient.  Every element is read
// and written by the same thread, so the in-place form needs no ordering beyond the barriers of the reductions.
constexpr int SOFT_TPB = 1024;
__global__ __launch_bounds__(SOFT_TPB) void ce_soft_kernel(const float* logits, long ld, const float* __restrict__ logq, long ldq,
                                                           const int64_t* __restrict__ tgt, float lambda, float* __restrict__ loss,
                                                           float* __restrict__ nll, float* __restrict__ soft,
                                                           float* __restrict__ kl, float* __restrict__ lse_out, float* dlogits,
                                                           float gscale, int V, int vec) {
  __shared__ float red[3][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  const float* y = logq + row * ldq;
  float m = -INFINITY, l = 0.f, Q = 0.f, qz = 0.f;
  const int V4 = vec ? (V & ~3) : 0;
  for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + j), u = *reinterpret_cast<const float4*>(y + j);
    const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (mx > m) { l *= __expf(m - mx); m = mx; }
    if (m > -INFINITY) l += __expf(v.x - m) + __expf(v.y - m) + __expf(v.z - m) + __expf(v.w - m);
    const float q0 = __expf(u.x), q1 = __expf(u.y), q2 = __expf(u.z), q3 = __expf(u.w);
    Q += (q0 + q1) + (q2 + q3);
    qz += ((q0 > 0.f ? q0 * v.x : 0.f) + (q1 > 0.f ? q1 * v.y : 0.f)) + ((q2 > 0.f ? q2 * v.z : 0.f) + (q3 > 0.f ? q3 * v.w : 0.f));
  }
  for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) {
    const float v = x[j], q = __expf(y[j]);
    if (v > m) { l *= __expf(m - v); m = v; }
    if (m > -INFINITY) l += __expf(v - m);
    Q += q;
    qz += q > 0.f ? q * v : 0.f;
  }
  const long t = tgt[row];
  const bool valid = t >= 0 && t < V;
  const float xt = valid ? x[t] : 0.f;  // read before any in-place gradient write (the reductions below have barriers)
  float M_ = m;
  row_fold<ROW_MAX>(red, M_);
  l = m == -INFINITY ? 0.f : l * __expf(m - M_);
  row_fold<ROW_SUM, ROW_EACH>(red, l, Q, qz);
  const float lse = M_ + __logf(l);
  const SoftCoef c = soft_coef(lambda, valid, Q, gscale);
  float* d = dlogits ? dlogits + row * ld : nullptr;
  float k = 0.f;
  for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + j), u = *reinterpret_cast<const float4*>(y + j);
    float4 g;
    k += (soft_elem(v.x, u.x, lse, c, g.x) + soft_elem(v.y, u.y, lse, c, g.y)) +
         (soft_elem(v.z, u.z, lse, c, g.z) + soft_elem(v.w, u.w, lse, c, g.w));
    if (d) {
      if (valid && t >= j && t < j + 4) {
        if (t == j) g.x -= c.t; else if (t == j + 1) g.y -= c.t; else if (t == j + 2) g.z -= c.t; else g.w -= c.t;
      }
      *reinterpret_cast<float4*>(d + j) = g;
    }
  }
  for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) {
    float g;
    k += soft_elem(x[j], y[j], lse, c, g);
    if (d) d[j] = (valid && j == t) ? g - c.t : g;
  }
  row_fold<ROW_SUM>(red, k);
  if (threadIdx.x == 0) {
    const float n = valid ? lse - xt : 0.f, s = Q * lse - qz;
    loss[row] = (1.f - lambda) * n + lambda * s;
    if (nll) nll[row] = n;
    if (soft) soft[row] = s;
    if (kl) kl[row] = k;
    if (lse_out) lse_out[row] = lse;
  }
}

// ---- top-k teacher targets: the same loss against a SPARSE row per token, K (id, logq) pairs (blm_ce_soft_topk_fwd_bwd) ----
// Thread j < K owns entry j of its row for the whole kernel: it reads the pair once, gathers z[ids_j] BEFORE the first
// barrier (so before any in-place gradient store of any thread), contributes q_j, q_j z_j and the KL term to the row's sums,
// and -- behind a barrier that follows the dense sweep's stores -- OVERWRITES column ids_j with the full gradient of that
// column, formed from the values it holds: Q p - q_j and, where ids_j is also the target, the one-hot term too.  No thread
// reads a gradient back, no atomics; with duplicate live ids the last writer wins (unspecified, in bounds).
struct TopkEntry {
  unsigned id;  // 0xFFFFFFFF: not live
  float l, q, z;
};
__device__ __forceinline__ TopkEntry topk_entry(const int* __restrict__ ids, const float* __restrict__ logq, const float* x, int K, int V) {
  TopkEntry e = {0xFFFFFFFFu, 0.f, 0.f, 0.f};
  if ((int)threadIdx.x < K) {
    const int id = ids[threadIdx.x];
    if (id >= 0 && id < V) {
      e.id = (unsigned)id;
      e.l = logq[threadIdx.x];
      e.q = __expf(e.l);
      e.z = x[id];
    }
  }
  return e;
}
__device__ __forceinline__ float topk_kl(const TopkEntry& e, float lse) { return e.q > 0.f ? e.q * (e.l - (e.z - lse)) : 0.f; }
__device__ __forceinline__ void topk_fix(const TopkEntry& e, float lse, const SoftCoef& c, unsigned tu, float* d) {
  if (e.id != 0xFFFFFFFFu) d[e.id] = (c.p * __expf(e.z - lse) - c.q * e.q) - (tu == e.id ? c.t : 0.f);
}
__device__ __forceinline__ void topk_finish(long row, bool valid, float xt, float lse, float Q, float qz, float k, float lambda,
                                            float* __restrict__ loss, float* __restrict__ nll, float* __restrict__ soft,
                                            float* __restrict__ kl, float* __restrict__ lse_out) {
  const float n = valid ? lse - xt : 0.f, s = Q * lse - qz;
  loss[row] = (1.f - lambda) * n + lambda * s;
  if (nll) nll[row] = n;
  if (soft) soft[row] = s;
  if (kl) kl[row] = k;
  if (lse_out) lse_out[row] = lse;
}

// The logit row held in registers as in ce_soft_row_kernel, and no second dense row beside it: NV = 3 / 9 / 16 as the hard-label
// ce_row_kernel, V <= 65536.  Requires V >= 4, ld a multiple of 4 and 16-byte aligned logits / dlogits (the entry point
// selects); ids / logq rows are read one element per thread and need no alignment.  logits / dlogits may alias.
template <int NV>
__global__ __launch_bounds__(1024) void ce_topk_row_kernel(const float* logits, long ld, const int* __restrict__ ids,
                                                           const float* __restrict__ logq, long ldk, int K,
                                                           const int64_t* __restrict__ tgt, float lambda, float* __restrict__ loss,
                                                           float* __restrict__ nll, float* __restrict__ soft,
                                                           float* __restrict__ kl, float* __restrict__ lse_out, float* dlogits,
                                                           float gscale, int V) {
  __shared__ float red[3][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  const unsigned t0 = threadIdx.x * 4u, Vu = (unsigned)V;
  float4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {  // whole quads only; a quad outside the row reads quad 0 and is skipped wherever it is used
    const unsigned j = t0 + 4096u * i;
    v[i] = *reinterpret_cast<const float4*>(x + (j + 3 < Vu ? j : 0u));
  }
  const unsigned je = (Vu & ~3u) + threadIdx.x;  // this thread's column behind the whole quads, if je < V
  const bool extra = je < Vu;
  const float ze = extra ? x[je] : -INFINITY;
  const TopkEntry e = topk_entry(ids + row * ldk, logq + row * ldk, x, K, V);
  const long t = tgt[row];
  const bool valid = t >= 0 && t < V;
  const float xt = valid ? x[t] : 0.f;  // as e.z: read before any in-place gradient write (the reductions below have barriers)
  const unsigned tu = valid ? (unsigned)t : 0xFFFFFFFFu;
  float m = ze;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
  }
  float M_ = m;
  row_fold<ROW_MAX>(red, M_);
  float l = __expf(ze - M_);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    l += __expf(v[i].x - M_) + __expf(v[i].y - M_) + __expf(v[i].z - M_) + __expf(v[i].w - M_);
  }
  float Q = e.q, qz = e.q > 0.f ? e.q * e.z : 0.f;
  row_fold<ROW_SUM, ROW_EACH>(red, l, Q, qz);
  const float lse = M_ + __logf(l);
  const SoftCoef c = soft_coef(lambda, valid, Q, gscale);
  float k = topk_kl(e, lse);
  row_fold<ROW_SUM>(red, k);
  if (dlogits) {
    float* d = dlogits + row * ld;
    if (extra) d[je] = c.p * __expf(ze - lse) - (tu == je ? c.t : 0.f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const unsigned j = t0 + 4096u * i;
      if (!(j + 3 < Vu)) continue;
      float4 g;
      g.x = c.p * __expf(v[i].x - lse) - (tu == j ? c.t : 0.f);
      g.y = c.p * __expf(v[i].y - lse) - (tu == j + 1 ? c.t : 0.f);
      g.z = c.p * __expf(v[i].z - lse) - (tu == j + 2 ? c.t : 0.f);
      g.w = c.p * __expf(v[i].w - lse) - (tu == j + 3 ? c.t : 0.f);
      *reinterpret_cast<float4*>(d + j) = g;
    }
    __syncthreads();  // every dense store of the row is behind this barrier; the K columns of the teacher are written after it
    topk_fix(e, lse, c, tu, d);
  }
  if (threadIdx.x == 0) topk_finish(row, valid, xt, lse, Q, qz, k, lambda, loss, nll, soft, kl, lse_out);
}

// Any V, any stride, any alignment: ce_soft_kernel's two sweeps over the logit row alone.
__global__ __launch_bounds__(SOFT_TPB) void ce_topk_kernel(const float* logits, long ld, const int* __restrict__ ids,
                                                           const float* __restrict__ logq, long ldk, int K,
                                                           const int64_t* __restrict__ tgt, float lambda, float* __restrict__ loss,
                                                           float* __restrict__ nll, float* __restrict__ soft,
                                                           float* __restrict__ kl, float* __restrict__ lse_out, float* dlogits,
                                                           float gscale, int V, int vec) {
  __shared__ float red[3][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  float m = -INFINITY, l = 0.f;
  const int V4 = vec ? (V & ~3) : 0;
  for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + j);
    const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (mx > m) { l *= __expf(m - mx); m = mx; }
    if (m > -INFINITY) l += __expf(v.x - m) + __expf(v.y - m) + __expf(v.z - m) + __expf(v.w - m);
  }
  for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) {
    const float v = x[j];
    if (v > m) { l *= __expf(m - v); m = v; }
    if (m > -INFINITY) l += __expf(v - m);
  }
  const TopkEntry e = topk_entry(ids + row * ldk, logq + row * ldk, x, K, V);
  const long t = tgt[row];
  const bool valid = t >= 0 && t < V;
  const float xt = valid ? x[t] : 0.f;  // as e.z: read before any in-place gradient write (the reductions below have barriers)
  const unsigned tu = valid ? (unsigned)t : 0xFFFFFFFFu;
  float M_ = m;
  row_fold<ROW_MAX>(red, M_);
  l = m == -INFINITY ? 0.f : l * __expf(m - M_);
  float Q = e.q, qz = e.q > 0.f ? e.q * e.z : 0.f;
  row_fold<ROW_SUM, ROW_EACH>(red, l, Q, qz);
  const float lse = M_ + __logf(l);
  const SoftCoef c = soft_coef(lambda, valid, Q, gscale);
  float k = topk_kl(e, lse);
  row_fold<ROW_SUM>(red, k);
  if (dlogits) {
    float* d = dlogits + row * ld;
    for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {  // each element read and written by the same thread
      const float4 v = *reinterpret_cast<const float4*>(x + j);
      const unsigned ju = (unsigned)j;
      float4 g;
      g.x = c.p * __expf(v.x - lse) - (tu == ju ? c.t : 0.f);
      g.y = c.p * __expf(v.y - lse) - (tu == ju + 1 ? c.t : 0.f);
      g.z = c.p * __expf(v.z - lse) - (tu == ju + 2 ? c.t : 0.f);
      g.w = c.p * __expf(v.w - lse) - (tu == ju + 3 ? c.t : 0.f);
      *reinterpret_cast<float4*>(d + j) = g;
    }
    for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) d[j] = c.p * __expf(x[j] - lse) - (tu == (unsigned)j ? c.t : 0.f);
    __syncthreads();  // as in ce_topk_row_kernel
    topk_fix(e, lse, c, tu, d);
  }
  if (threadIdx.x == 0) topk_finish(row, valid, xt, lse, Q, qz, k, lambda, loss, nll, soft, kl, lse_out);
}

// ---- distillation temperature: blm_ce_soft_temp_fwd_bwd / blm_ce_soft_topk_temp_fwd_bwd (definitions: include/bayeslm.h) ----
// The hard term stays at temperature 1, the soft term compares softmax(beta z) with the teacher raised to beta and renormalised
// over its live entries, so one read of a row has to give both softmax(z) and softmax(beta z).  Three rounds per row:
//   1. max z and max live l                                          (one row_fold: one barrier pair)
//   2. sum exp(z - m), s_b = sum exp(beta (z - m)), Z = sum e_v, A = sum e_v (z_v - m),  e_v = exp(beta (l_v - ml))
//                                                                    (one row_fold: one barrier pair)
//   3. the KL terms and the gradient, every exponent formed from the max-shifted values: log p = (z - m) - log sum,
//      log p~ = beta (z - m) - log s_b, log q~ = beta (l - ml) - log Z
// soft = log s_b - beta A / Z, which is lse_b - beta sum q~ z with the beta m of both terms cancelled before it is rounded.
// The untempered kernels above are not touched: temperature 1 launches them.

struct TempRow {  // a row's constants of round 3, the same in every lane
  float beta, m, logl, logs, ml, logZ;  // log p = (z - m) - logl,  log p~ = beta (z - m) - logs,  log q~ = beta (l - ml) - logZ
  float hard, soft;                     // gradient = hard (p - onehot) + soft (p~ - q~)
  float lse, sft;                       // outputs: the temperature-1 lse and the unscaled soft term
  bool valid;
};
// rounds 1 and 2 leave (m, ml) and the four sums; a row without a live teacher entry (ml = -inf) has soft = kl = 0 and no soft
// gradient: ml and log Z are set to 0 there so that log q~ = beta (-inf - 0) - 0 = -inf, q~ = 0, without an inf - inf
__device__ __forceinline__ TempRow temp_row(float beta, float m, float ml, float l, float sb, float Z, float A, float lambda,
                                            float scale, bool valid, float gscale) {
  const bool has_q = ml > -INFINITY;
  TempRow r;
  r.beta = beta;
  r.m = m;
  r.logl = __logf(l);
  r.logs = __logf(sb);
  r.ml = has_q ? ml : 0.f;
  r.logZ = has_q ? __logf(Z) : 0.f;
  r.hard = valid ? (1.f - lambda) * gscale : 0.f;
  r.soft = has_q ? lambda * scale * beta * gscale : 0.f;
  r.lse = m + r.logl;
  r.sft = has_q ? r.logs - beta * (A / Z) : 0.f;
  r.valid = valid;
  return r;
}
// one (z, l) pair of round 2: its terms of the four sums
__device__ __forceinline__ void temp_acc(float z, float l, float beta, float m, float mls, float& sl, float& sb, float& Z, float& A) {
  const float a = z - m, e = __expf(beta * (l - mls));
  sl += __expf(a);
  sb += __expf(beta * a);
  Z += e;
  A += e > 0.f ? e * a : 0.f;
}
// one element of round 3: its KL term (returned) and its gradient (g), the one-hot term apart
__device__ __forceinline__ float temp_elem(float z, float l, const TempRow& r, float& g) {
  const float a = z - r.m, lb = r.beta * a - r.logs, lt = r.beta * (l - r.ml) - r.logZ;
  const float qt = __expf(lt);
  g = r.hard * __expf(a - r.logl) + r.soft * (__expf(lb) - qt);
  return qt > 0.f ? qt * (lt - lb) : 0.f;
}
// ... of a column the teacher row does not hold (top-k: every column of the dense sweep)
__device__ __forceinline__ float temp_grad(float z, const TempRow& r) {
  const float a = z - r.m;
  return r.hard * __expf(a - r.logl) + r.soft * __expf(r.beta * a - r.logs);
}
__device__ __forceinline__ void temp_finish(long row, const TempRow& r, float xt, float k, float lambda, float scale,
                                            float* __restrict__ loss, float* __restrict__ nll, float* __restrict__ soft,
                                            float* __restrict__ kl, float* __restrict__ lse_out) {
  const float n = r.valid ? r.lse - xt : 0.f;
  loss[row] = (1.f - lambda) * n + lambda * scale * r.sft;
  if (nll) nll[row] = n;
  if (soft) soft[row] = r.sft;
  if (kl) kl[row] = k;
  if (lse_out) lse_out[row] = r.lse;
}

// ce_soft_row_kernel with a temperature: both rows in registers, each read from memory once; same requirements.
template <int NV>
__global__ __launch_bounds__(1024) void ce_soft_temp_row_kernel(const float* logits, long ld, const float* __restrict__ logq, long ldq,
                                                                const int64_t* __restrict__ tgt, float lambda, float beta, float scale,
                                                                float* __restrict__ loss, float* __restrict__ nll,
                                                                float* __restrict__ soft, float* __restrict__ kl,
                                                                float* __restrict__ lse_out, float* dlogits, float gscale, int V) {
  __shared__ float red[4][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  const float* y = logq + row * ldq;
  const unsigned t0 = threadIdx.x * 4u, Vu = (unsigned)V;
  float4 v[NV], u[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {  // whole quads only; a quad outside the row reads quad 0 and is skipped wherever it is used
    const unsigned j = t0 + 4096u * i;
    const unsigned js = j + 3 < Vu ? j : 0u;
    v[i] = *reinterpret_cast<const float4*>(x + js);
    u[i] = *reinterpret_cast<const float4*>(y + js);
  }
  const unsigned je = (Vu & ~3u) + threadIdx.x;  // this thread's column behind the whole quads, if je < V
  const bool extra = je < Vu;
  const float ze = extra ? x[je] : -INFINITY, le = extra ? y[je] : -INFINITY;
  const long t = tgt[row];
  const bool valid = t >= 0 && t < V;
  const float xt = valid ? x[t] : 0.f;  // read before any in-place gradient write (the reductions below have barriers)
  const unsigned tu = valid ? (unsigned)t : 0xFFFFFFFFu;
  float m = ze, ml = le;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
    ml = fmaxf(ml, fmaxf(fmaxf(u[i].x, u[i].y), fmaxf(u[i].z, u[i].w)));
  }
  row_fold<ROW_MAX, ROW_UNIFORM>(red, m, ml);
  const float mls = ml > -INFINITY ? ml : 0.f;
  float sl = 0.f, sb = 0.f, Z = 0.f, A = 0.f;
  temp_acc(ze, le, beta, m, mls, sl, sb, Z, A);  // ze = le = -inf without an extra column: four zeros
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    temp_acc(v[i].x, u[i].x, beta, m, mls, sl, sb, Z, A);
    temp_acc(v[i].y, u[i].y, beta, m, mls, sl, sb, Z, A);
    temp_acc(v[i].z, u[i].z, beta, m, mls, sl, sb, Z, A);
    temp_acc(v[i].w, u[i].w, beta, m, mls, sl, sb, Z, A);
  }
  row_fold<ROW_SUM, ROW_UNIFORM | ROW_EACH>(red, sl, sb, Z, A);
  const TempRow r = temp_row(beta, m, ml, sl, sb, Z, A, lambda, scale, valid, gscale);
  float* d = dlogits ? dlogits + row * ld : nullptr;
  float ge;
  float k = temp_elem(ze, le, r, ge);
  if (d && extra) d[je] = tu == je ? ge - r.hard : ge;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const unsigned j = t0 + 4096u * i;
    if (!(j + 3 < Vu)) continue;
    float4 g;
    k += (temp_elem(v[i].x, u[i].x, r, g.x) + temp_elem(v[i].y, u[i].y, r, g.y)) +
         (temp_elem(v[i].z, u[i].z, r, g.z) + temp_elem(v[i].w, u[i].w, r, g.w));
    if (d) {
      g.x -= tu == j ? r.hard : 0.f;
      g.y -= tu == j + 1 ? r.hard : 0.f;
      g.z -= tu == j + 2 ? r.hard : 0.f;
      g.w -= tu == j + 3 ? r.hard : 0.f;
      *reinterpret_cast<float4*>(d + j) = g;
    }
  }
  row_fold<ROW_SUM>(red, k);
  if (threadIdx.x == 0) temp_finish(row, r, xt, k, lambda, scale, loss, nll, soft, kl, lse_out);
}

// Any V, any stride, any alignment: the three rounds as three sweeps over both rows (the second and third from L2 / the
// Infinity Cache).  Every element is read and written by the same thread, and the first store lies behind the barriers of
// round 2, so the in-place form needs no further ordering.
__global__ __launch_bounds__(SOFT_TPB) void ce_soft_temp_kernel(const float* logits, long ld, const float* __restrict__ logq, long ldq,
                                                                const int64_t* __restrict__ tgt, float lambda, float beta, float scale,
                                                                float* __restrict__ loss, float* __restrict__ nll,
                                                                float* __restrict__ soft, float* __restrict__ kl,
                                                                float* __restrict__ lse_out, float* dlogits, float gscale, int V,
                                                                int vec) {
  __shared__ float red[4][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  const float* y = logq + row * ldq;
  const int V4 = vec ? (V & ~3) : 0;
  float m = -INFINITY, ml = -INFINITY;
  for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + j), u = *reinterpret_cast<const float4*>(y + j);
    m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    ml = fmaxf(ml, fmaxf(fmaxf(u.x, u.y), fmaxf(u.z, u.w)));
  }
  for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) {
    m = fmaxf(m, x[j]);
    ml = fmaxf(ml, y[j]);
  }
  const long t = tgt[row];
  const bool valid = t >= 0 && t < V;
  const float xt = valid ? x[t] : 0.f;  // read before any in-place gradient write
  row_fold<ROW_MAX, ROW_UNIFORM>(red, m, ml);
  const float mls = ml > -INFINITY ? ml : 0.f;
  float sl = 0.f, sb = 0.f, Z = 0.f, A = 0.f;
  for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + j), u = *reinterpret_cast<const float4*>(y + j);
    temp_acc(v.x, u.x, beta, m, mls, sl, sb, Z, A);
    temp_acc(v.y, u.y, beta, m, mls, sl, sb, Z, A);
    temp_acc(v.z, u.z, beta, m, mls, sl, sb, Z, A);
    temp_acc(v.w, u.w, beta, m, mls, sl, sb, Z, A);
  }
  for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) temp_acc(x[j], y[j], beta, m, mls, sl, sb, Z, A);
  row_fold<ROW_SUM, ROW_UNIFORM | ROW_EACH>(red, sl, sb, Z, A);
  const TempRow r = temp_row(beta, m, ml, sl, sb, Z, A, lambda, scale, valid, gscale);
  float* d = dlogits ? dlogits + row * ld : nullptr;
  float k = 0.f;
  for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + j), u = *reinterpret_cast<const float4*>(y + j);
    float4 g;
    k += (temp_elem(v.x, u.x, r, g.x) + temp_elem(v.y, u.y, r, g.y)) + (temp_elem(v.z, u.z, r, g.z) + temp_elem(v.w, u.w, r, g.w));
    if (d) {
      if (valid && t >= j && t < j + 4) {
        if (t == j) g.x -= r.hard; else if (t == j + 1) g.y -= r.hard; else if (t == j + 2) g.z -= r.hard; else g.w -= r.hard;
      }
      *reinterpret_cast<float4*>(d + j) = g;
    }
  }
  for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) {
    float g;
    k += temp_elem(x[j], y[j], r, g);
    if (d) d[j] = (valid && j == t) ? g - r.hard : g;
  }
  row_fold<ROW_SUM>(red, k);
  if (threadIdx.x == 0) temp_finish(row, r, xt, k, lambda, scale, loss, nll, soft, kl, lse_out);
}

// top-k with a temperature.  Thread j < K owns entry j as in the untempered kernels; an entry is LIVE when its id lies in
// [0, V) and its logq is above -inf.  An entry with a good id and logq = -inf takes no part in the sums (l = -inf gives e = 0)
// and still overwrites its column -- with the value the dense sweep wrote there.
struct TempEntry {
  unsigned id;  // 0xFFFFFFFF: an empty slot
  float l, z;   // l = -inf, z = 0 in an empty slot
};
__device__ __forceinline__ TempEntry temp_entry(const int* __restrict__ ids, const float* __restrict__ logq, const float* x, int K, int V) {
  TempEntry e = {0xFFFFFFFFu, -INFINITY, 0.f};
  if ((int)threadIdx.x < K) {
    const int id = ids[threadIdx.x];
    if (id >= 0 && id < V) {
      e.id = (unsigned)id;
      e.l = logq[threadIdx.x];
      e.z = x[id];
    }
  }
  return e;
}
__device__ __forceinline__ void temp_fix(const TempEntry& e, const TempRow& r, unsigned tu, float* d) {
  if (e.id == 0xFFFFFFFFu) return;
  float g;
  temp_elem(e.z, e.l, r, g);
  d[e.id] = g - (tu == e.id ? r.hard : 0.f);
}

template <int NV>
__global__ __launch_bounds__(1024) void ce_topk_temp_row_kernel(const float* logits, long ld, const int* __restrict__ ids,
                                                                const float* __restrict__ logq, long ldk, int K,
                                                                const int64_t* __restrict__ tgt, float lambda, float beta, float scale,
                                                                float* __restrict__ loss, float* __restrict__ nll,
                                                                float* __restrict__ soft, float* __restrict__ kl,
                                                                float* __restrict__ lse_out, float* dlogits, float gscale, int V) {
  __shared__ float red[4][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  const unsigned t0 = threadIdx.x * 4u, Vu = (unsigned)V;
  float4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {  // whole quads only; a quad outside the row reads quad 0 and is skipped wherever it is used
    const unsigned j = t0 + 4096u * i;
    v[i] = *reinterpret_cast<const float4*>(x + (j + 3 < Vu ? j : 0u));
  }
  const unsigned je = (Vu & ~3u) + threadIdx.x;  // this thread's column behind the whole quads, if je < V
  const bool extra = je < Vu;
  const float ze = extra ? x[je] : -INFINITY;
  const TempEntry e = temp_entry(ids + row * ldk, logq + row * ldk, x, K, V);
  const long t = tgt[row];
  const bool valid = t >= 0 && t < V;
  const float xt = valid ? x[t] : 0.f;  // as e.z: read before any in-place gradient write (the reductions below have barriers)
  const unsigned tu = valid ? (unsigned)t : 0xFFFFFFFFu;
  float m = ze, ml = e.l;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
  }
  row_fold<ROW_MAX, ROW_UNIFORM>(red, m, ml);
  const float mls = ml > -INFINITY ? ml : 0.f;
  float sl = __expf(ze - m), sb = __expf(beta * (ze - m));
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    sl += __expf(v[i].x - m) + __expf(v[i].y - m) + __expf(v[i].z - m) + __expf(v[i].w - m);
    sb += __expf(beta * (v[i].x - m)) + __expf(beta * (v[i].y - m)) + __expf(beta * (v[i].z - m)) + __expf(beta * (v[i].w - m));
  }
  float Z = __expf(beta * (e.l - mls)), A = Z > 0.f ? Z * (e.z - m) : 0.f;
  row_fold<ROW_SUM, ROW_UNIFORM | ROW_EACH>(red, sl, sb, Z, A);
  const TempRow r = temp_row(beta, m, ml, sl, sb, Z, A, lambda, scale, valid, gscale);
  float gu, k = temp_elem(e.z, e.l, r, gu);
  row_fold<ROW_SUM>(red, k);
  if (dlogits) {
    float* d = dlogits + row * ld;
    if (extra) d[je] = temp_grad(ze, r) - (tu == je ? r.hard : 0.f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const unsigned j = t0 + 4096u * i;
      if (!(j + 3 < Vu)) continue;
      float4 g;
      g.x = temp_grad(v[i].x, r) - (tu == j ? r.hard : 0.f);
      g.y = temp_grad(v[i].y, r) - (tu == j + 1 ? r.hard : 0.f);
      g.z = temp_grad(v[i].z, r) - (tu == j + 2 ? r.hard : 0.f);
      g.w = temp_grad(v[i].w, r) - (tu == j + 3 ? r.hard : 0.f);
      *reinterpret_cast<float4*>(d + j) = g;
    }
    __syncthreads();  // every dense store of the row is behind this barrier; the K columns of the teacher are written after it
    temp_fix(e, r, tu, d);
  }
  if (threadIdx.x == 0) temp_finish(row, r, xt, k, lambda, scale, loss, nll, soft, kl, lse_out);
}

// Any V, any stride, any alignment: ce_topk_kernel's two sweeps, the online pass carrying both sum exp(z - m) and s_b.
__global__ __launch_bounds__(SOFT_TPB) void ce_topk_temp_kernel(const float* logits, long ld, const int* __restrict__ ids,
                                                                const float* __restrict__ logq, long ldk, int K,
                                                                const int64_t* __restrict__ tgt, float lambda, float beta, float scale,
                                                                float* __restrict__ loss, float* __restrict__ nll,
                                                                float* __restrict__ soft, float* __restrict__ kl,
                                                                float* __restrict__ lse_out, float* dlogits, float gscale, int V,
                                                                int vec) {
  __shared__ float red[4][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  float mt = -INFINITY, sl = 0.f, sb = 0.f;
  const int V4 = vec ? (V & ~3) : 0;
  for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + j);
    const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (mx > mt) { sl *= __expf(mt - mx); sb *= __expf(beta * (mt - mx)); mt = mx; }
    if (mt > -INFINITY) {
      sl += __expf(v.x - mt) + __expf(v.y - mt) + __expf(v.z - mt) + __expf(v.w - mt);
      sb += __expf(beta * (v.x - mt)) + __expf(beta * (v.y - mt)) + __expf(beta * (v.z - mt)) + __expf(beta * (v.w - mt));
    }
  }
  for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) {
    const float v = x[j];
    if (v > mt) { sl *= __expf(mt - v); sb *= __expf(beta * (mt - v)); mt = v; }
    if (mt > -INFINITY) { sl += __expf(v - mt); sb += __expf(beta * (v - mt)); }
  }
  const TempEntry e = temp_entry(ids + row * ldk, logq + row * ldk, x, K, V);
  const long t = tgt[row];
  const bool valid = t >= 0 && t < V;
  const float xt = valid ? x[t] : 0.f;  // as e.z: read before any in-place gradient write (the reductions below have barriers)
  const unsigned tu = valid ? (unsigned)t : 0xFFFFFFFFu;
  float m = mt, ml = e.l;
  row_fold<ROW_MAX, ROW_UNIFORM>(red, m, ml);
  const float mls = ml > -INFINITY ? ml : 0.f;
  sl = mt == -INFINITY ? 0.f : sl * __expf(mt - m);
  sb = mt == -INFINITY ? 0.f : sb * __expf(beta * (mt - m));
  float Z = __expf(beta * (e.l - mls)), A = Z > 0.f ? Z * (e.z - m) : 0.f;
  row_fold<ROW_SUM, ROW_UNIFORM | ROW_EACH>(red, sl, sb, Z, A);
  const TempRow r = temp_row(beta, m, ml, sl, sb, Z, A, lambda, scale, valid, gscale);
  float gu, k = temp_elem(e.z, e.l, r, gu);
  row_fold<ROW_SUM>(red, k);
  if (dlogits) {
    float* d = dlogits + row * ld;
    for (int j = threadIdx.x * 4; j < V4; j += SOFT_TPB * 4) {  // each element read and written by the same thread
      const float4 v = *reinterpret_cast<const float4*>(x + j);
      const unsigned ju = (unsigned)j;
      float4 g;
      g.x = temp_grad(v.x, r) - (tu == ju ? r.hard : 0.f);
      g.y = temp_grad(v.y, r) - (tu == ju + 1 ? r.hard : 0.f);
      g.z = temp_grad(v.z, r) - (tu == ju + 2 ? r.hard : 0.f);
      g.w = temp_grad(v.w, r) - (tu == ju + 3 ? r.hard : 0.f);
      *reinterpret_cast<float4*>(d + j) = g;
    }
    for (int j = V4 + threadIdx.x; j < V; j += SOFT_TPB) d[j] = temp_grad(x[j], r) - (tu == (unsigned)j ? r.hard : 0.f);
    __syncthreads();  // as in ce_topk_temp_row_kernel
    temp_fix(e, r, tu, d);
  }
  if (threadIdx.x == 0) temp_finish(row, r, xt, k, lambda, scale, loss, nll, soft, kl, lse_out);
}

// deterministic single-block sum: out += sum(x[0..n))  (the fixed-order loss_sum of blm_ce_fwd_bwd)
__global__ __launch_bounds__(1024) void soft_sum_kernel(const float* __restrict__ x, long n, float* out) {
  __shared__ float red[16];
  float a = 0.f;
  for (long i = threadIdx.x; i < n; i += 1024) a += x[i];
  const float t = block_sum<16>(a, red);
  if (threadIdx.x == 0) out[0] += t;
}

}  // namespace blm

using namespace blm;

// The gradient may be written over the logits it is the gradient of, element for element, and over nothing else read here.
static int dlogits_args(const char* fn, const Span& d, const Span& z, const Span& q, const Span* ids) {
  if (ids && overlaps(d, *ids)) return blm_fail(BLM_ERR_INVALID, "%s: dlogits overlaps ids", fn);
  if (overlaps(d, q)) return blm_fail(BLM_ERR_INVALID, "%s: dlogits overlaps logq", fn);
  if (!in_place_or_disjoint(d, z))
    return blm_fail(BLM_ERR_INVALID, "%s: dlogits overlaps logits without being logits itself (in place means dlogits == logits)", fn);
  return BLM_OK;
}

// The argument checks of the dense entry points, under the name `fn` of the one that was called -> BLM_OK to go on.
static int soft_args(const char* fn, const float* logits, int64_t ld, const float* logq, int64_t ldq, const int64_t* tgt, float lambda,
                     const float* loss, const float* dlogits, int M, int V) {
  if (!logits || !logq || !tgt || !loss) return blm_fail(BLM_ERR_INVALID, "%s: logits, logq, tgt and loss are required", fn);
  if (M < 0 || V <= 0) return blm_fail(BLM_ERR_INVALID, "%s: M = %d, V = %d: M >= 0 and V > 0 expected", fn, M, V);
  if (ld < V || ldq < V || !extents_ok({M, ld}) || !extents_ok({M, ldq}))
    return blm_fail(BLM_ERR_INVALID, "%s: row strides ld = %lld, ldq = %lld must be >= V = %d (and M x stride an addressable extent)", fn,
                    (long long)ld, (long long)ldq, V);
  if (!(lambda >= 0.f && lambda <= 1.f)) return blm_fail(BLM_ERR_INVALID, "%s: lambda = %g outside [0, 1]", fn, (double)lambda);
  if (M == 0 || !dlogits) return BLM_OK;
  return dlogits_args(fn, span_of(dlogits, M, ld, V), span_of(logits, M, ld, V), span_of(logq, M, ldq, V), nullptr);
}
// ... and what the tempered entry points refuse beside: beta = 1 / T and the factor on the soft term
static int temp_args(const char* fn, float beta, float soft_scale) {
  if (!(beta > 0.f) || !std::isfinite(beta)) return blm_fail(BLM_ERR_INVALID, "%s: beta = %g: a finite inverse temperature > 0 expected", fn, (double)beta);
  if (!(soft_scale >= 0.f) || !std::isfinite(soft_scale))
    return blm_fail(BLM_ERR_INVALID, "%s: soft_scale = %g: a finite factor >= 0 expected", fn, (double)soft_scale);
  return BLM_OK;
}
// The argument checks of the top-k entry points, under the name `fn` of the one that was called -> BLM_OK to go on.
static int topk_args(const char* fn, const float* logits, int64_t ld, const int32_t* ids, const float* logq, int64_t ldk, int K,
                     const int64_t* tgt, float lambda, const float* loss, const float* dlogits, int M, int V) {
  const char* missing = !logits ? "logits" : !ids ? "ids" : !logq ? "logq" : !tgt ? "tgt" : !loss ? "loss" : nullptr;
  if (missing) return blm_fail(BLM_ERR_INVALID, "%s: %s is NULL (logits, ids, logq, tgt and loss are required)", fn, missing);
  if (M < 0 || V <= 0) return blm_fail(BLM_ERR_INVALID, "%s: M = %d, V = %d: M >= 0 and V > 0 expected", fn, M, V);
  if (K < 1 || K > BLM_TOPK_MAX) return blm_fail(BLM_ERR_INVALID, "%s: K = %d outside [1, BLM_TOPK_MAX = %d]", fn, K, BLM_TOPK_MAX);
  if (ld < V || !extents_ok({M, ld}))
    return blm_fail(BLM_ERR_INVALID, "%s: row stride ld = %lld must be >= V = %d (and M x ld an addressable extent)", fn, (long long)ld, V);
  if (ldk < K || !extents_ok({M, ldk}))
    return blm_fail(BLM_ERR_INVALID, "%s: row stride ldk = %lld must be >= K = %d (and M x ldk an addressable extent)", fn, (long long)ldk, K);
  if (!(lambda >= 0.f && lambda <= 1.f)) return blm_fail(BLM_ERR_INVALID, "%s: lambda = %g outside [0, 1]", fn, (double)lambda);
  if (M == 0 || !dlogits) return BLM_OK;
  const Span i = span_of(ids, M, ldk, K);  // 4-byte ids
  return dlogits_args(fn, span_of(dlogits, M, ld, V), span_of(logits, M, ld, V), span_of(logq, M, ldk, K), &i);
}

// The launch of all four entry points.  `vec`: every matrix the kernels read or write by float4 (the logits, the gradient and,
// DENSE, the teacher row) is 16-byte aligned at a row stride that is a multiple of 4.  Then the row-held form at the first of
// NV = 3, 9 and -- top-k only, which holds one row and not two -- 16 quads per thread that covers V, else the sweep; the dense
// entry points' second rung has never asked for V >= 4.  row(nv) and sweep(vec) launch the entry point's own kernels.  Last the
// fixed-order loss_sum, if asked for.
template <int NV>
using nv_c = std::integral_constant<int, NV>;
template <bool DENSE, class Row, class Sweep>
static int soft_launch(const float* logits, int64_t ld, const float* logq, int64_t ldq, const float* dlogits, int V, const float* loss,
                       int M, float* loss_sum, hipStream_t st, Row row, Sweep sweep) {
  const bool vec = (ld & 3) == 0 && (!DENSE || ((ldq & 3) == 0 && aligned16(logq))) && aligned16(logits, dlogits);
  const bool quad = vec && V >= 4;
  if (quad && V <= 4096 * 3) row(nv_c<3>{});
  else if ((DENSE ? vec : quad) && V <= 4096 * 9) row(nv_c<9>{});
  else if (!DENSE && quad && V <= 4096 * 16) {
    if constexpr (!DENSE) row(nv_c<16>{});
  } else sweep(vec ? 1 : 0);
  BLM_HIP(hipGetLastError());
  if (loss_sum) {
    hipLaunchKernelGGL(soft_sum_kernel, dim3(1), dim3(1024), 0, st, loss, (long)M, loss_sum);
    BLM_HIP(hipGetLastError());
  }
  return BLM_OK;
}

extern "C" int blm_ce_soft_fwd_bwd(const float* logits, int64_t ld, const float* logq, int64_t ldq, const int64_t* tgt, float lambda,
                                   float* loss, float* nll, float* soft, float* kl, float* lse, float* loss_sum, float* dlogits,
                                   float grad_scale, int M, int V, void* stream) {
  if (const int bad = soft_args("blm_ce_soft_fwd_bwd", logits, ld, logq, ldq, tgt, lambda, loss, dlogits, M, V)) return bad;
  if (M == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return soft_launch<true>(
      logits, ld, logq, ldq, dlogits, V, loss, M, loss_sum, st,
      [&](auto nv) {
        hipLaunchKernelGGL(ce_soft_row_kernel<decltype(nv)::value>, dim3(M), dim3(1024), 0, st, logits, (long)ld, logq, (long)ldq, tgt,
                           lambda, loss, nll, soft, kl, lse, dlogits, grad_scale, V);
      },
      [&](int vec) {
        hipLaunchKernelGGL(ce_soft_kernel, dim3(M), dim3(SOFT_TPB), 0, st, logits, (long)ld, logq, (long)ldq, tgt, lambda, loss, nll, soft,
                           kl, lse, dlogits, grad_scale, V, vec);
      });
}

extern "C" int blm_ce_soft_temp_fwd_bwd(const float* logits, int64_t ld, const float* logq, int64_t ldq, const int64_t* tgt, float lambda,
                                        float beta, float soft_scale, float* loss, float* nll, float* soft, float* kl, float* lse,
                                        float* loss_sum, float* dlogits, float grad_scale, int M, int V, void* stream) {
  if (const int bad = soft_args("blm_ce_soft_temp_fwd_bwd", logits, ld, logq, ldq, tgt, lambda, loss, dlogits, M, V)) return bad;
  if (const int bad = temp_args("blm_ce_soft_temp_fwd_bwd", beta, soft_scale)) return bad;
  if (M == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return soft_launch<true>(
      logits, ld, logq, ldq, dlogits, V, loss, M, loss_sum, st,
      [&](auto nv) {
        hipLaunchKernelGGL(ce_soft_temp_row_kernel<decltype(nv)::value>, dim3(M), dim3(1024), 0, st, logits, (long)ld, logq, (long)ldq, tgt,
                           lambda, beta, soft_scale, loss, nll, soft, kl, lse, dlogits, grad_scale, V);
      },
      [&](int vec) {
        hipLaunchKernelGGL(ce_soft_temp_kernel, dim3(M), dim3(SOFT_TPB), 0, st, logits, (long)ld, logq, (long)ldq, tgt, lambda, beta,
                           soft_scale, loss, nll, soft, kl, lse, dlogits, grad_scale, V, vec);
      });
}

extern "C" int blm_ce_soft_topk_fwd_bwd(const float* logits, int64_t ld, const int32_t* ids, const float* logq, int64_t ldk, int K,
                                        const int64_t* tgt, float lambda, float* loss, float* nll, float* soft, float* kl, float* lse,
                                        float* loss_sum, float* dlogits, float grad_scale, int M, int V, void* stream) {
  if (const int bad = topk_args("blm_ce_soft_topk_fwd_bwd", logits, ld, ids, logq, ldk, K, tgt, lambda, loss, dlogits, M, V)) return bad;
  if (M == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return soft_launch<false>(
      logits, ld, nullptr, 0, dlogits, V, loss, M, loss_sum, st,
      [&](auto nv) {
        hipLaunchKernelGGL(ce_topk_row_kernel<decltype(nv)::value>, dim3(M), dim3(1024), 0, st, logits, (long)ld, ids, logq, (long)ldk, K,
                           tgt, lambda, loss, nll, soft, kl, lse, dlogits, grad_scale, V);
      },
      [&](int vec) {
        hipLaunchKernelGGL(ce_topk_kernel, dim3(M), dim3(SOFT_TPB), 0, st, logits, (long)ld, ids, logq, (long)ldk, K, tgt, lambda, loss,
                           nll, soft, kl, lse, dlogits, grad_scale, V, vec);
      });
}

extern "C" int blm_ce_soft_topk_temp_fwd_bwd(const float* logits, int64_t ld, const int32_t* ids, const float* logq, int64_t ldk, int K,
                                             const int64_t* tgt, float lambda, float beta, float soft_scale, float* loss, float* nll,
                                             float* soft, float* kl, float* lse, float* loss_sum, float* dlogits, float grad_scale, int M,
                                             int V, void* stream) {
  if (const int bad = topk_args("blm_ce_soft_topk_temp_fwd_bwd", logits, ld, ids, logq, ldk, K, tgt, lambda, loss, dlogits, M, V)) return bad;
  if (const int bad = temp_args("blm_ce_soft_topk_temp_fwd_bwd", beta, soft_scale)) return bad;
  if (M == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return soft_launch<false>(
      logits, ld, nullptr, 0, dlogits, V, loss, M, loss_sum, st,
      [&](auto nv) {
        hipLaunchKernelGGL(ce_topk_temp_row_kernel<decltype(nv)::value>, dim3(M), dim3(1024), 0, st, logits, (long)ld, ids, logq, (long)ldk,
                           K, tgt, lambda, beta, soft_scale, loss, nll, soft, kl, lse, dlogits, grad_scale, V);
      },
      [&](int vec) {
        hipLaunchKernelGGL(ce_topk_temp_kernel, dim3(M), dim3(SOFT_TPB), 0, st, logits, (long)ld, ids, logq, (long)ldk, K, tgt, lambda,
                           beta, soft_scale, loss, nll, soft, kl, lse, dlogits, grad_scale, V, vec);
      });
}
