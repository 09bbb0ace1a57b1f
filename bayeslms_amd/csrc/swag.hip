// SWAG (Maddox, Garipov, Izmailov, Vetrov, Wilson, NeurIPS 2019): a Gaussian over all weights fitted to the SGD iterates, and
// the model average over weight samples whose decoders differ.  Definitions: include/bayeslm.h.
//
//   blm_swag_collect     Welford update of mean and m2 by one iterate, and one row of the deviation ring   (5 or 6 streams)
//   blm_swag_sample      J = 1, 2, 4, 8 samples from ONE read of mean, m2 and the k_live deviation rows    (2 + K read, J written)
//   blm_logp_avg_accum   log-softmax of a row of logits folded into the running log-mean-exp of the samples
//
// The first two are memory-bound streaming kernels in dyneval.hip's shape: one grid-stride pass of 16-byte loads and stores over
// the aligned body and a scalar tail, a grid of at most SWAG_GRID workgroups of 256 lanes; pointers or strides that are not
// 16-byte aligned take the scalar path for the whole array.  Fused multiply-adds are written out and contraction is off, so an
// element gets the same bits on either path, and a sample the same bits in every form and slot.  The third is one workgroup per
// row; its sums are folded in a fixed order without atomics: the same bits in every run.
#include <cmath>

#include "blm_device.h"
#include "blm_host.h"

namespace blm {
namespace {

constexpr int SWAG_TPB = 256;
constexpr int SWAG_GRID = 2048;

inline int swag_grid(long n) {
  const long blocks = (n / 4 + SWAG_TPB - 1) / SWAG_TPB;  // one float4 per lane and trip
  return (int)(blocks < 1 ? 1 : (blocks > SWAG_GRID ? SWAG_GRID : blocks));
}

// ---------------------------------------------------------------- collect
// d = th - mean; mean' = mean + d * inv; m2' = m2 + d * (th - mean'); deviation = th - mean'.  FIRST: mean and m2 are not read.
template <bool FIRST>
__device__ __forceinline__ void collect_one(float th, float& mean, float& m2, float& dev, float inv) {
#pragma clang fp contract(off)
  if (FIRST) {
    mean = th, m2 = 0.f, dev = 0.f;
  } else {
    const float d = th - mean;
    const float mn = mean + d * inv;
    dev = th - mn;
    m2 = m2 + d * dev;
    mean = mn;
  }
}

template <bool FIRST, bool DEV>
__global__ __launch_bounds__(SWAG_TPB) void swag_collect_kernel(const float* __restrict__ theta, float* __restrict__ mean,
                                                                float* __restrict__ m2, float* __restrict__ dev, long n,
                                                                float inv) {
  const long n4 = aligned16(theta, mean, m2, dev) ? (n >> 2) : 0;
  const long stride = (long)gridDim.x * SWAG_TPB, first = (long)blockIdx.x * SWAG_TPB + threadIdx.x;
  for (long i = first; i < n4; i += stride) {
    const float4 tv = reinterpret_cast<const float4*>(theta)[i];
    float4 mv = make_float4(0.f, 0.f, 0.f, 0.f), qv = mv, dv;
    if (!FIRST) {
      mv = reinterpret_cast<const float4*>(mean)[i];
      qv = reinterpret_cast<const float4*>(m2)[i];
    }
    collect_one<FIRST>(tv.x, mv.x, qv.x, dv.x, inv); collect_one<FIRST>(tv.y, mv.y, qv.y, dv.y, inv);
    collect_one<FIRST>(tv.z, mv.z, qv.z, dv.z, inv); collect_one<FIRST>(tv.w, mv.w, qv.w, dv.w, inv);
    reinterpret_cast<float4*>(mean)[i] = mv;
    reinterpret_cast<float4*>(m2)[i] = qv;
    if (DEV) reinterpret_cast<float4*>(dev)[i] = dv;
  }
  for (long i = (n4 << 2) + first; i < n; i += stride) {
    float m = 0.f, q = 0.f, d;
    if (!FIRST) m = mean[i], q = m2[i];
    collect_one<FIRST>(theta[i], m, q, d, inv);
    mean[i] = m;
    m2[i] = q;
    if (DEV) dev[i] = d;
  }
}

// ---------------------------------------------------------------- sample
// One element of slot j, in this order whatever the form:
//   sd = sqrt(max(m2 * inv_n, floor));  base = fma(a * sd, z1, mean);  low = fma(D[k], z2[k], low) for k ascending from low = 0;
//   out = fma(b, low, base)
struct SwagCoef {
  float a, b, inv_n, floor;
};

__device__ __forceinline__ float swag_sd(float m2, const SwagCoef& c) {
#pragma clang fp contract(off)
  return c.a * __builtin_sqrtf(fmaxf(m2 * c.inv_n, c.floor));
}

__device__ __forceinline__ void fma4(float4& acc, const float4& d, float z) {
  acc.x = __builtin_fmaf(d.x, z, acc.x); acc.y = __builtin_fmaf(d.y, z, acc.y);
  acc.z = __builtin_fmaf(d.z, z, acc.z); acc.w = __builtin_fmaf(d.w, z, acc.w);
}

// J slots, of which the first `count` are live: the others are neither computed nor written.  z2 holds count rows of k_live
// floats; an index into it is uniform over the workgroup, so its values arrive by scalar loads and stay in scalar registers.
template <int J>
__global__ __launch_bounds__(SWAG_TPB) void swag_sample_kernel(float* __restrict__ out, long ld_out, const float* __restrict__ mean,
                                                               const float* __restrict__ m2, const float* __restrict__ dev,
                                                               long ld_dev, int k_live, const float* __restrict__ z2, long n,
                                                               blm_swag_draw draw) {
#pragma clang fp contract(off)
  const SwagCoef c = {draw.a, draw.b, draw.inv_n, draw.var_floor};
  const int count = draw.count;
  const bool vec = aligned16(out, mean, m2, k_live > 0 ? dev : nullptr) && ((ld_out | (k_live > 0 ? ld_dev : 0)) & 3) == 0;
  const long n4 = vec ? (n >> 2) : 0;
  const long stride = (long)gridDim.x * SWAG_TPB, first = (long)blockIdx.x * SWAG_TPB + threadIdx.x;
  for (long i = first; i < n4; i += stride) {
    float4 low[J];
#pragma unroll
    for (int j = 0; j < J; ++j) low[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 mv = reinterpret_cast<const float4*>(mean)[i];
    const float4 qv = reinterpret_cast<const float4*>(m2)[i];
    int k = 0;
    for (; k + 4 <= k_live; k += 4) {  // four deviation rows in flight per lane
      const float4 d0 = reinterpret_cast<const float4*>(dev + (long)k * ld_dev)[i];
      const float4 d1 = reinterpret_cast<const float4*>(dev + (long)(k + 1) * ld_dev)[i];
      const float4 d2 = reinterpret_cast<const float4*>(dev + (long)(k + 2) * ld_dev)[i];
      const float4 d3 = reinterpret_cast<const float4*>(dev + (long)(k + 3) * ld_dev)[i];
#pragma unroll
      for (int j = 0; j < J; ++j)
        if (j < count) {
          const float* z = z2 + j * k_live + k;
          fma4(low[j], d0, z[0]); fma4(low[j], d1, z[1]); fma4(low[j], d2, z[2]); fma4(low[j], d3, z[3]);
        }
    }
    for (; k < k_live; ++k) {
      const float4 d0 = reinterpret_cast<const float4*>(dev + (long)k * ld_dev)[i];
#pragma unroll
      for (int j = 0; j < J; ++j)
        if (j < count) fma4(low[j], d0, z2[j * k_live + k]);
    }
    const float4 sd = make_float4(swag_sd(qv.x, c), swag_sd(qv.y, c), swag_sd(qv.z, c), swag_sd(qv.w, c));
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (j < count) {
        const blm_rng r = {draw.rng.seed, draw.rng.stream, draw.sample_id[j]};
        const float4 z1 = philox_normal4(r, (uint64_t)i);
        float4 o;
        o.x = __builtin_fmaf(c.b, low[j].x, __builtin_fmaf(sd.x, z1.x, mv.x));
        o.y = __builtin_fmaf(c.b, low[j].y, __builtin_fmaf(sd.y, z1.y, mv.y));
        o.z = __builtin_fmaf(c.b, low[j].z, __builtin_fmaf(sd.z, z1.z, mv.z));
        o.w = __builtin_fmaf(c.b, low[j].w, __builtin_fmaf(sd.w, z1.w, mv.w));
        reinterpret_cast<float4*>(out + (long)j * ld_out)[i] = o;
      }
  }
  for (long i = (n4 << 2) + first; i < n; i += stride) {
    float low[J];
#pragma unroll
    for (int j = 0; j < J; ++j) low[j] = 0.f;
    for (int k = 0; k < k_live; ++k) {
      const float d = dev[(long)k * ld_dev + i];
#pragma unroll
      for (int j = 0; j < J; ++j)
        if (j < count) low[j] = __builtin_fmaf(d, z2[j * k_live + k], low[j]);
    }
    const float mv = mean[i], sd = swag_sd(m2[i], c);
    const int e = (int)(i & 3);
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (j < count) {
        const blm_rng r = {draw.rng.seed, draw.rng.stream, draw.sample_id[j]};
        const float4 z = philox_normal4(r, (uint64_t)i >> 2);
        const float z1 = e == 0 ? z.x : (e == 1 ? z.y : (e == 2 ? z.z : z.w));
        out[(long)j * ld_out + i] = __builtin_fmaf(c.b, low[j], __builtin_fmaf(sd, z1, mv));
      }
  }
}

// ---------------------------------------------------------------- log-mean-exp over the samples
// exp(d) and exp(d) d of one column, d = x - max; a column at -inf adds nothing to either (p log p -> 0 at p = 0), also while
// the running max of a sweep is still -inf itself, where x - max would be NaN
__device__ __forceinline__ void lavg_term(float x, float M, float& l, float& u) {
  const bool fin = x > -INFINITY;  // then M >= x is finite too
  const float d = x - M, e = fin ? __expf(d) : 0.f;
  l += e;
  u += fin ? e * d : 0.f;
}

// the running log of the sum of the samples' probabilities, one column: both at -inf stays -inf
__device__ __forceinline__ float lavg_fold(float acc, float lp) {
  const float mx = fmaxf(acc, lp);
  return mx == -INFINITY ? mx : mx + log1pf(__expf(-fabsf(acc - lp)));
}

struct LavgTail {
  const int64_t* tgt;
  float* hsum;
  float* nll_s;
  int rows, s, last;
  float log_s;
};

// what lane 0 writes for its row: the sample's entropy into hsum, the target's NLL into nll_s
__device__ __forceinline__ void lavg_row_out(const LavgTail& t, long row, const float* x, int V, float lse, float H) {
  if (t.hsum) t.hsum[row] = t.s == 0 ? H : t.hsum[row] + H;
  if (t.nll_s) {
    const long tg = t.tgt[row];
    t.nll_s[(long)t.s * t.rows + row] = (tg >= 0 && tg < V) ? lse - x[tg] : 0.f;  // blm_ce_fwd_bwd's rule
  }
}

__device__ __forceinline__ float lavg_col(float x, float lse, float prev, const LavgTail& t) {
  float r = x - lse;
  if (t.s != 0) r = lavg_fold(prev, r);
  if (t.last) r -= t.log_s;
  return r;
}

// The row held in registers, ce_row_kernel's form: 1024 threads x NV float4 cover V <= 4096 NV, the logits are read once.
// Requires ld, ld_acc multiples of 4 and 16-byte aligned bases.
template <int NV>
__global__ __launch_bounds__(1024) void logp_avg_row_kernel(const float* __restrict__ logits, long ld, float* __restrict__ acc,
                                                            long ld_acc, int V, LavgTail t) {
  __shared__ float red[2][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  float* a = acc + row * ld_acc;
  const int t0 = threadIdx.x * 4;
  float4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = t0 + 4096 * i;
    if (j + 3 < V) v[i] = *reinterpret_cast<const float4*>(x + j);
    else {
      v[i].x = j < V ? x[j] : -INFINITY;
      v[i].y = j + 1 < V ? x[j + 1] : -INFINITY;
      v[i].z = j + 2 < V ? x[j + 2] : -INFINITY;
      v[i].w = -INFINITY;
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV; ++i) m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
  float M_ = m;
  row_fold<ROW_MAX>(red, M_);
  float l = 0.f, u = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    lavg_term(v[i].x, M_, l, u); lavg_term(v[i].y, M_, l, u); lavg_term(v[i].z, M_, l, u); lavg_term(v[i].w, M_, l, u);
  }
  row_fold<ROW_SUM>(red, l, u);
  const float logl = __logf(l), lse = M_ + logl;
  if (threadIdx.x == 0) lavg_row_out(t, row, x, V, lse, logl - u / l);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = t0 + 4096 * i;
    if (j + 3 < V) {
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t.s != 0) p = *reinterpret_cast<const float4*>(a + j);
      p.x = lavg_col(v[i].x, lse, p.x, t); p.y = lavg_col(v[i].y, lse, p.y, t);
      p.z = lavg_col(v[i].z, lse, p.z, t); p.w = lavg_col(v[i].w, lse, p.w, t);
      *reinterpret_cast<float4*>(a + j) = p;
    } else {
      if (j < V) a[j] = lavg_col(v[i].x, lse, t.s != 0 ? a[j] : 0.f, t);
      if (j + 1 < V) a[j + 1] = lavg_col(v[i].y, lse, t.s != 0 ? a[j + 1] : 0.f, t);
      if (j + 2 < V) a[j + 2] = lavg_col(v[i].z, lse, t.s != 0 ? a[j + 2] : 0.f, t);
    }
  }
}

// Two sweeps for every other shape: an online (max, sum exp, sum exp d) per lane, merged at the workgroup's max; then the
// columns again.  16-byte accesses where both matrices allow them, scalar otherwise.
__global__ __launch_bounds__(1024) void logp_avg_sweep_kernel(const float* __restrict__ logits, long ld, float* __restrict__ acc,
                                                              long ld_acc, int V, LavgTail t) {
  __shared__ float red[2][16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  float* a = acc + row * ld_acc;
  const bool vec = ((ld | ld_acc) & 3) == 0 && aligned16(logits, acc);
  const int V4 = vec ? (V & ~3) : 0;
  float m = -INFINITY, l = 0.f, u = 0.f;
  auto rescale = [&](float mx) {  // the state re-expressed for a max mx > m
    if (m > -INFINITY) {
      const float d = m - mx, f = __expf(d);
      u = f * (u + d * l);
      l *= f;
    }
    m = mx;
  };
  for (int j = threadIdx.x * 4; j < V4; j += 4096) {
    const float4 w = *reinterpret_cast<const float4*>(x + j);
    const float mx = fmaxf(fmaxf(w.x, w.y), fmaxf(w.z, w.w));
    if (mx > m) rescale(mx);
    lavg_term(w.x, m, l, u); lavg_term(w.y, m, l, u); lavg_term(w.z, m, l, u); lavg_term(w.w, m, l, u);
  }
  for (int j = V4 + threadIdx.x; j < V; j += 1024) {
    const float w = x[j];
    if (w > m) rescale(w);
    lavg_term(w, m, l, u);
  }
  float M_ = m;
  row_fold<ROW_MAX>(red, M_);
  if (m < M_) rescale(M_);  // a lane that saw no finite column keeps l = u = 0
  row_fold<ROW_SUM>(red, l, u);
  const float logl = __logf(l), lse = M_ + logl;
  if (threadIdx.x == 0) lavg_row_out(t, row, x, V, lse, logl - u / l);
  for (int j = threadIdx.x * 4; j < V4; j += 4096) {
    const float4 w = *reinterpret_cast<const float4*>(x + j);
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t.s != 0) p = *reinterpret_cast<const float4*>(a + j);
    p.x = lavg_col(w.x, lse, p.x, t); p.y = lavg_col(w.y, lse, p.y, t);
    p.z = lavg_col(w.z, lse, p.z, t); p.w = lavg_col(w.w, lse, p.w, t);
    *reinterpret_cast<float4*>(a + j) = p;
  }
  for (int j = V4 + threadIdx.x; j < V; j += 1024) a[j] = lavg_col(x[j], lse, t.s != 0 ? a[j] : 0.f, t);
}

inline bool swag_finite_nonneg(float v) { return v >= 0.f && v <= 3.402823466e38f; }

}  // namespace
}  // namespace blm

extern "C" int blm_swag_collect(const float* theta, float* mean, float* m2, float* dev_row, int64_t n_floats, int64_t count,
                                void* stream) {
  if (!theta || !mean || !m2) return blm_fail(BLM_ERR_INVALID, "blm_swag_collect: null operand");
  if (n_floats < 0 || n_floats > blm::kMaxElems)
    return blm_fail(BLM_ERR_INVALID, "blm_swag_collect: n_floats = %lld outside 0..2^40", (long long)n_floats);
  if (count < 0 || count >= (1LL << 24))
    return blm_fail(BLM_ERR_INVALID, "blm_swag_collect: count = %lld outside 0..2^24-1 (1 / (count + 1) is formed in fp32)",
                    (long long)count);
  if (n_floats == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(blm::swag_grid((long)n_floats)), block(blm::SWAG_TPB);
  const long n = (long)n_floats;
  const float inv = 1.0f / (float)(count + 1);
  if (count == 0) {
    if (dev_row) hipLaunchKernelGGL((blm::swag_collect_kernel<true, true>), grid, block, 0, st, theta, mean, m2, dev_row, n, inv);
    else hipLaunchKernelGGL((blm::swag_collect_kernel<true, false>), grid, block, 0, st, theta, mean, m2, dev_row, n, inv);
  } else {
    if (dev_row) hipLaunchKernelGGL((blm::swag_collect_kernel<false, true>), grid, block, 0, st, theta, mean, m2, dev_row, n, inv);
    else hipLaunchKernelGGL((blm::swag_collect_kernel<false, false>), grid, block, 0, st, theta, mean, m2, dev_row, n, inv);
  }
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_swag_sample(float* out, int64_t ld_out, const float* mean, const float* m2, const float* dev, int64_t ld_dev,
                               int k_live, const float* z2, int64_t n_floats, const blm_swag_draw* draw, void* stream) {
  if (!out || !mean || !m2 || !draw) return blm_fail(BLM_ERR_INVALID, "blm_swag_sample: null operand");
  if (draw->abi_version != BLM_ABI_VERSION)
    return blm_fail(BLM_ERR_ABI, "blm_swag_sample: draw abi_version %u != %u", draw->abi_version, (unsigned)BLM_ABI_VERSION);
  if (n_floats < 0 || n_floats > blm::kMaxElems)
    return blm_fail(BLM_ERR_INVALID, "blm_swag_sample: n_floats = %lld outside 0..2^40", (long long)n_floats);
  if (draw->count < 1 || draw->count > BLM_SWAG_DRAWS_MAX)
    return blm_fail(BLM_ERR_INVALID, "blm_swag_sample: count %d outside 1..%d", (int)draw->count, BLM_SWAG_DRAWS_MAX);
  if (k_live < 0 || k_live > BLM_SWAG_RANK_MAX)
    return blm_fail(BLM_ERR_INVALID, "blm_swag_sample: k_live %d outside 0..%d", k_live, BLM_SWAG_RANK_MAX);
  if (k_live > 0 && (!dev || !z2)) return blm_fail(BLM_ERR_INVALID, "blm_swag_sample: k_live %d without dev or z2", k_live);
  if (ld_out < n_floats || ld_out > blm::kMaxElems || (k_live > 0 && (ld_dev < n_floats || ld_dev > blm::kMaxElems)))
    return blm_fail(BLM_ERR_INVALID, "blm_swag_sample: ld_out %lld / ld_dev %lld below n_floats %lld or beyond 2^40", (long long)ld_out,
                    (long long)ld_dev, (long long)n_floats);
  if (!blm::swag_finite_nonneg(draw->a) || !blm::swag_finite_nonneg(draw->b) || !blm::swag_finite_nonneg(draw->var_floor) ||
      !(draw->inv_n > 0.f) || !blm::swag_finite_nonneg(draw->inv_n))
    return blm_fail(BLM_ERR_INVALID, "blm_swag_sample: a %g, b %g, floor %g must be finite and >= 0, inv_n %g finite and > 0",
                    (double)draw->a, (double)draw->b, (double)draw->var_floor, (double)draw->inv_n);
  if (n_floats == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(blm::swag_grid((long)n_floats)), block(blm::SWAG_TPB);
  const long n = (long)n_floats, lo = (long)ld_out, ldd = (long)ld_dev;
  blm::for_slots(draw->count, [&](auto J) {
    hipLaunchKernelGGL((blm::swag_sample_kernel<J()>), grid, block, 0, st, out, lo, mean, m2, dev, ldd, k_live, z2, n, *draw);
  });
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_logp_avg_accum(const float* logits, int64_t ld, float* acc, int64_t ld_acc, const int64_t* targets, int rows,
                                  int V, int s, int S, float* hsum, float* nll_s, void* stream) {
  if (!logits || !acc) return blm_fail(BLM_ERR_INVALID, "blm_logp_avg_accum: null operand");
  if ((targets == nullptr) != (nll_s == nullptr))
    return blm_fail(BLM_ERR_INVALID, "blm_logp_avg_accum: targets and nll_s go together");
  if (rows < 0 || V <= 0 || ld < V || ld_acc < V || !blm::extents_ok({rows, V}) || ld > blm::kMaxElems || ld_acc > blm::kMaxElems)
    return blm_fail(BLM_ERR_INVALID, "blm_logp_avg_accum: bad shape (rows %d, V %d, ld %lld, ld_acc %lld)", rows, V, (long long)ld,
                    (long long)ld_acc);
  if (S < 1 || S > BLM_SWAG_SAMPLES_MAX || s < 0 || s >= S)
    return blm_fail(BLM_ERR_INVALID, "blm_logp_avg_accum: sample %d of %d (S in 1..%d, 0 <= s < S)", s, S, BLM_SWAG_SAMPLES_MAX);
  if (rows == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const blm::LavgTail t = {targets, hsum, nll_s, rows, s, s == S - 1 ? 1 : 0, (float)std::log((double)S)};
  const bool vec = ((ld | ld_acc) & 3) == 0 && blm::aligned16(logits, acc);
  if (vec && V <= 4096 * 3)
    hipLaunchKernelGGL(blm::logp_avg_row_kernel<3>, dim3(rows), dim3(1024), 0, st, logits, (long)ld, acc, (long)ld_acc, V, t);
  else if (vec && V <= 4096 * 9)
    hipLaunchKernelGGL(blm::logp_avg_row_kernel<9>, dim3(rows), dim3(1024), 0, st, logits, (long)ld, acc, (long)ld_acc, V, t);
  else
    hipLaunchKernelGGL(blm::logp_avg_sweep_kernel, dim3(rows), dim3(1024), 0, st, logits, (long)ld, acc, (long)ld_acc, V, t);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
