// Last-layer Laplace posterior for the decoder (MacKay 1992; Kristiadi, Hein, Hennig 2020; Daxberger et al. 2021): the three row
// kernels of bayeslms_amd/laplace.py and engine.fit_laplace / evaluate_laplace.  Definitions: include/bayeslm.h.
//
//   blm_laplace_curvature   a = p (1 - p) of a row of logits, the diagonal GGN factor          (one read, one write)
//   blm_laplace_row_stats   blm_row_stats' figures of y = link(z, var), formed in registers    (z and var read once)
//   blm_laplace_mc_rows     the model average over S logit samples z + sqrt(var) eps           (no S x V intermediate)
//
// Vector ALU, one workgroup per row.  Every fold runs in a fixed order (xor butterfly inside a wave, then the waves in turn
// through LDS) without atomics, fused multiply-adds are written out and contraction is off: the same bits in every run, and in
// blm_laplace_mc_rows on the 16-byte and on the scalar path alike and for a sample whatever runs beside it.
#include <cmath>

#include "blm_device.h"
#include "blm_host.h"
#include "blm_rowstat.h"

namespace blm {
namespace {

constexpr int LP_TPB = 256;
constexpr int LP_WAVES = LP_TPB / 64;

// columns j .. j + 3 of a row of V: one 16-byte load where the row allows it and the quad is whole, else guarded scalars
__device__ __forceinline__ float4 lp_load4(const float* p, int j, int V, bool vec, float fill) {
  if (vec && j + 3 < V) return *reinterpret_cast<const float4*>(p + j);
  float4 r;
  r.x = j < V ? p[j] : fill;
  r.y = j + 1 < V ? p[j + 1] : fill;
  r.z = j + 2 < V ? p[j + 2] : fill;
  r.w = j + 3 < V ? p[j + 3] : fill;
  return r;
}

// ---------------------------------------------------------------- curvature
// exp(x - M) of one column for the row's sum; a column at -inf adds nothing, a NaN makes the sum NaN
__device__ __forceinline__ float curv_term(float x, float M) { return x == -INFINITY ? 0.f : __expf(x - M); }

__device__ __forceinline__ float curv_one(float x, float lse) {
#pragma clang fp contract(off)
  const float p = x == -INFINITY ? 0.f : __expf(x - lse);
  return __builtin_fmaf(-p, p, p);
}

// The row held in registers, logp_avg_row_kernel's form: 1024 threads x NV float4 cover V <= 4096 NV; the logits are read once
// and a is written once.  Requires ld and lda multiples of 4 and 16-byte aligned bases.  In place (a == x): every load of the
// row is behind the reductions' barriers before the first store.
template <int NV>
__global__ __launch_bounds__(1024) void curv_row_kernel(const float* logits, long ld, float* out, long lda, int V) {
  __shared__ float red[16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  float* a = out + row * lda;
  const int t0 = threadIdx.x * 4;
  float4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = lp_load4(x, t0 + 4096 * i, V, true, -INFINITY);
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV; ++i) m = fmaxf(m, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
  const float M_ = block_max<16>(m, red);
  float l = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    l += curv_term(v[i].x, M_); l += curv_term(v[i].y, M_); l += curv_term(v[i].z, M_); l += curv_term(v[i].w, M_);
  }
  l = block_sum<16>(l, red);
  const float lse = M_ + logf(l);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = t0 + 4096 * i;
    if (j >= V) continue;
    float4 p;  // a column past V holds -inf and gives 0: the pad columns of the last quad (lda % 4 == 0: they exist)
    p.x = curv_one(v[i].x, lse); p.y = curv_one(v[i].y, lse); p.z = curv_one(v[i].z, lse); p.w = curv_one(v[i].w, lse);
    *reinterpret_cast<float4*>(a + j) = p;
  }
}

// Two sweeps for every other shape: an online (max, sum exp) per lane, merged at the workgroup's max, then the columns again
// (the second read of a row this workgroup just streamed).  16-byte accesses where both matrices allow them.
__global__ __launch_bounds__(1024) void curv_sweep_kernel(const float* logits, long ld, float* out, long lda, int V, int vec) {
  __shared__ float red[16];
  const long row = blockIdx.x;
  const float* x = logits + row * ld;
  float* a = out + row * lda;
  const int V4 = vec ? (V & ~3) : 0;
  float m = -INFINITY, l = 0.f;
  auto rescale = [&](float mx) {
    if (m > -INFINITY) l *= __expf(m - mx);
    m = mx;
  };
  for (int j = threadIdx.x * 4; j < V4; j += 4096) {
    const float4 w = *reinterpret_cast<const float4*>(x + j);
    const float mx = fmaxf(fmaxf(w.x, w.y), fmaxf(w.z, w.w));
    if (mx > m) rescale(mx);
    l += curv_term(w.x, m); l += curv_term(w.y, m); l += curv_term(w.z, m); l += curv_term(w.w, m);
  }
  for (int j = V4 + threadIdx.x; j < V; j += 1024) {
    const float w = x[j];
    if (w > m) rescale(w);
    l += curv_term(w, m);
  }
  const float M_ = block_max<16>(m, red);
  if (m < M_) rescale(M_);  // a lane that saw no finite column keeps l = 0 (or its NaN)
  l = block_sum<16>(l, red);
  const float lse = M_ + logf(l);
  for (int j = threadIdx.x * 4; j < V4; j += 4096) {
    const float4 w = *reinterpret_cast<const float4*>(x + j);
    float4 p;
    p.x = curv_one(w.x, lse); p.y = curv_one(w.y, lse); p.z = curv_one(w.z, lse); p.w = curv_one(w.w, lse);
    *reinterpret_cast<float4*>(a + j) = p;
  }
  for (int j = V4 + threadIdx.x; j < V; j += 1024) a[j] = curv_one(x[j], lse);
  const int Vq = (V + 3) & ~3;
  if (lda >= Vq && V + (int)threadIdx.x < Vq) a[V + threadIdx.x] = 0.f;
}

// ---------------------------------------------------------------- closed-form links
constexpr int LINK_PROBIT = 0, LINK_EXPEXP = 1;

// y of one column.  probit: z / sqrt(1 + (pi / 8) var), the reciprocal square root by v_rsq_f32; expexp: z + var / 2.
template <int LINK>
__device__ __forceinline__ float link_y(float z, float var) {
#pragma clang fp contract(off)
  if (LINK == LINK_PROBIT) return z * __builtin_amdgcn_rsqf(__builtin_fmaf(0.39269908169872414f, var, 1.0f));
  return __builtin_fmaf(0.5f, var, z);
}

// y = link(z, var) of the row's columns, formed in registers; the variance rides beside it
template <int LINK>
struct LinkCols {
  const float *zr, *vr;
  __device__ __forceinline__ float one(int c, float& var) const {
    var = vr[c];
    return link_y<LINK>(zr[c], var);
  }
  __device__ __forceinline__ float4 quad(int i, float4& vv) const {
    const float4 zz = reinterpret_cast<const float4*>(zr)[i];
    vv = reinterpret_cast<const float4*>(vr)[i];
    return make_float4(link_y<LINK>(zz.x, vv.x), link_y<LINK>(zz.y, vv.y), link_y<LINK>(zz.z, vv.z), link_y<LINK>(zz.w, vv.w));
  }
};

template <int LINK>
__global__ __launch_bounds__(LP_TPB) void laplace_row_stats_kernel(const float* z, long ldz, const float* var, long ldv,
                                                                   const int64_t* tgt, int V, int vec, float* nll, float* conf,
                                                                   float* entropy, int32_t* pred, int32_t* rank, float* vbar) {
  __shared__ RowAccW red[LP_WAVES];
  const int row = blockIdx.x;
  const LinkCols<LINK> src{z + (long)row * ldz, var + (long)row * ldv};
  const RowTarget t = row_target(tgt, row, V, src);
  RowAccW a{{}, -INFINITY, 0.f, 0.f, 0.f, kNone, 0, 0};
  const int n4 = vec ? (V >> 2) : 0;
  a = row_quads<LP_TPB>(a, src, n4, t);
  row_columns<LP_TPB>(a, src, 4 * n4 + threadIdx.x, V, t);  // the V % 4 last columns, or the whole row on the scalar path
  if (!row_state_fold<LP_TPB>(a, red)) return;
  row_finish(row, a, t, nll, conf, entropy, pred, rank);
  if (vbar) vbar[row] = a.bad ? NAN : a.w / a.s;
}

// ---------------------------------------------------------------- Monte-Carlo link
struct McArgs {
  const float* z;
  long ldz;
  const float* var;
  long ldv;
  const int64_t* tgt;
  int R, V, S, vec;
  uint64_t seed;
  uint32_t stream;
  long row0;
  float *bma_nll, *nll_s, *h_pred, *mi, *conf;
  int32_t *pred, *rank;
};

constexpr int MC_GROUP = 8;  // samples whose (max, sum) a lane carries through one sweep of the row

// z_s of the four columns of counter block `block`: fma(sd, eps, z).  A column past V holds z = -inf and sd = 0: -inf.
__device__ __forceinline__ float4 mc_sample4(const float4& z, const float4& sd, const McArgs& p, int s, uint64_t block) {
#pragma clang fp contract(off)
  const blm_rng r = {p.seed, p.stream, (uint32_t)s};
  const float4 e = philox_normal4(r, block);
  return make_float4(__builtin_fmaf(sd.x, e.x, z.x), __builtin_fmaf(sd.y, e.y, z.y), __builtin_fmaf(sd.z, e.z, z.z),
                     __builtin_fmaf(sd.w, e.w, z.w));
}

__device__ __forceinline__ float4 mc_sd4(const float4& v) {
  return make_float4(__builtin_sqrtf(v.x), __builtin_sqrtf(v.y), __builtin_sqrtf(v.z), __builtin_sqrtf(v.w));
}

__device__ __forceinline__ int mc_bad4(const float4& z, const float4& v, int j, int V) {
  int bad = 0;
  bad |= (j < V) && ((z.x != z.x) || !(v.x >= 0.f && v.x < INFINITY));
  bad |= (j + 1 < V) && ((z.y != z.y) || !(v.y >= 0.f && v.y < INFINITY));
  bad |= (j + 2 < V) && ((z.z != z.z) || !(v.z >= 0.f && v.z < INFINITY));
  bad |= (j + 3 < V) && ((z.w != z.w) || !(v.w >= 0.f && v.w < INFINITY));
  return bad;
}

__device__ __forceinline__ void mc_online4(float& m, float& l, const float4& x) {
#pragma clang fp contract(off)
  const float cm = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
  if (cm > m) {
    l = l * __expf(m - cm);  // m = -inf: l = 0 stays 0
    m = cm;
  }
  l = l + curv_term(x.x, m);
  l = l + curv_term(x.y, m);
  l = l + curv_term(x.z, m);
  l = l + curv_term(x.w, m);
}

__device__ __forceinline__ void mc_merge(float& m, float& l, float mb, float lb) {
#pragma clang fp contract(off)
  const float M = fmaxf(m, mb);
  const float fa = m == M ? 1.f : __expf(m - M), fb = mb == M ? 1.f : __expf(mb - M);
  l = l * fa + lb * fb;
  m = M;
}

// sum_s exp(z_s - lse_s) of a quad, s ascending: the same bits wherever it is called for that quad
__device__ __forceinline__ float4 mc_psum4(const float4& z, const float4& sd, const McArgs& p, uint64_t block, const float* lse) {
#pragma clang fp contract(off)
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
  for (int s = 0; s < p.S; ++s) {
    const float4 x = mc_sample4(z, sd, p, s, block);
    const float L = lse[s];
    sum.x = sum.x + __expf(x.x - L);
    sum.y = sum.y + __expf(x.y - L);
    sum.z = sum.z + __expf(x.z - L);
    sum.w = sum.w + __expf(x.w - L);
  }
  return sum;
}

struct McFold {
  float h, kl, mx;
  int am, cnt;
};

__device__ __forceinline__ void mc_fold_merge(McFold& a, const McFold& b) {
#pragma clang fp contract(off)
  if (b.mx > a.mx || (b.mx == a.mx && b.am < a.am)) {
    a.mx = b.mx;
    a.am = b.am;
  }
  a.h = a.h + b.h;
  a.kl = a.kl + b.kl;
  a.cnt += b.cnt;
}

// one column of the second sweep: pbar, its entropy term, the maximum and the rank count
__device__ __forceinline__ float mc_column(McFold& f, float pb, int c, int V, float pt, int tg) {
#pragma clang fp contract(off)
  if (c >= V) return 0.f;
  const float lp = pb > 0.f ? logf(pb) : 0.f;
  f.h = __builtin_fmaf(-pb, lp, f.h);
  if (pb > f.mx) {
    f.mx = pb;
    f.am = c;
  }
  f.cnt += (c != tg && (pb > pt || (pb == pt && c < tg))) ? 1 : 0;
  return lp;
}

__device__ __forceinline__ float mc_kl_term(float x, float L, float lp) {
#pragma clang fp contract(off)
  const float d = x - L, q = __expf(d);
  return q > 0.f ? q * (d - lp) : 0.f;
}

__global__ __launch_bounds__(LP_TPB) void laplace_mc_rows_kernel(McArgs p) {
#pragma clang fp contract(off)
  __shared__ float lse[BLM_LAPLACE_SAMPLES_MAX];
  __shared__ float red_m[LP_WAVES][MC_GROUP], red_l[LP_WAVES][MC_GROUP];
  __shared__ McFold red_f[LP_WAVES];
  __shared__ float pt_lds;
  const int row = blockIdx.x, V = p.V, S = p.S;
  const bool vec = p.vec != 0;
  const float* zr = p.z + (long)row * p.ldz;
  const float* vr = p.var + (long)row * p.ldv;
  const int nq = (V + 3) >> 2;
  const uint64_t blk0 = (uint64_t)(p.row0 + row) * (uint64_t)nq;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int bad = 0;

  // sweep 1: lse_s of every sample, MC_GROUP samples per pass over the row
  for (int g0 = 0; g0 < S; g0 += MC_GROUP) {
    float m[MC_GROUP], l[MC_GROUP];
#pragma unroll
    for (int j = 0; j < MC_GROUP; ++j) m[j] = -INFINITY, l[j] = 0.f;
    for (int q = threadIdx.x; q < nq; q += LP_TPB) {
      const float4 z4 = lp_load4(zr, 4 * q, V, vec, -INFINITY);
      const float4 v4 = lp_load4(vr, 4 * q, V, vec, 0.f);
      bad |= mc_bad4(z4, v4, 4 * q, V);
      const float4 sd = mc_sd4(v4);
#pragma unroll
      for (int j = 0; j < MC_GROUP; ++j)
        if (g0 + j < S) mc_online4(m[j], l[j], mc_sample4(z4, sd, p, g0 + j, blk0 + q));
    }
#pragma unroll
    for (int j = 0; j < MC_GROUP; ++j) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mc_merge(m[j], l[j], __shfl_xor(m[j], o, 64), __shfl_xor(l[j], o, 64));
      if (lane == 0) red_m[w][j] = m[j], red_l[w][j] = l[j];
    }
    __syncthreads();
    if (threadIdx.x < MC_GROUP && g0 + (int)threadIdx.x < S) {
      float M = red_m[0][threadIdx.x], Ls = red_l[0][threadIdx.x];
      for (int k = 1; k < LP_WAVES; ++k) mc_merge(M, Ls, red_m[k][threadIdx.x], red_l[k][threadIdx.x]);
      lse[g0 + threadIdx.x] = M + logf(Ls);
    }
    __syncthreads();
  }
  bad = __syncthreads_or(bad);

  // the target's pbar, by the function the second sweep uses for that quad (the same bits): one lane forms it, LDS hands it on
  const int64_t t64 = p.tgt ? p.tgt[row] : -1;
  const bool has_t = t64 >= 0 && t64 < V;
  const int tg = has_t ? (int)t64 : -1;
  const float inv_s = 1.0f / (float)S;
  if (threadIdx.x == 0) {
    float t = NAN;  // NaN compares false: nothing is counted without a target
    if (has_t) {
      const int tq = tg >> 2;
      const float4 z4 = lp_load4(zr, 4 * tq, V, vec, -INFINITY);
      const float4 sd = mc_sd4(lp_load4(vr, 4 * tq, V, vec, 0.f));
      t = comp(mc_psum4(z4, sd, p, blk0 + tq, lse), tg & 3) * inv_s;
      if (p.nll_s) {
#pragma unroll 1
        for (int s = 0; s < S; ++s)
          p.nll_s[(long)s * p.R + row] = bad ? NAN : lse[s] - comp(mc_sample4(z4, sd, p, s, blk0 + tq), tg & 3);
      }
    } else if (p.nll_s) {
      for (int s = 0; s < S; ++s) p.nll_s[(long)s * p.R + row] = NAN;
    }
    pt_lds = t;
  }
  __syncthreads();
  const float pt = pt_lds;

  // sweep 2: pbar of every column, then the KL terms of that column with the noise made again
  McFold f{0.f, 0.f, -INFINITY, 0x7fffffff, 0};
  for (int q = threadIdx.x; q < nq; q += LP_TPB) {
    const float4 z4 = lp_load4(zr, 4 * q, V, vec, -INFINITY);
    const float4 sd = mc_sd4(lp_load4(vr, 4 * q, V, vec, 0.f));
    const float4 sum = mc_psum4(z4, sd, p, blk0 + q, lse);
    const int c = 4 * q;
    float4 lp;
    lp.x = mc_column(f, sum.x * inv_s, c, V, pt, tg);
    lp.y = mc_column(f, sum.y * inv_s, c + 1, V, pt, tg);
    lp.z = mc_column(f, sum.z * inv_s, c + 2, V, pt, tg);
    lp.w = mc_column(f, sum.w * inv_s, c + 3, V, pt, tg);
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      const float4 x = mc_sample4(z4, sd, p, s, blk0 + q);
      const float L = lse[s];
      f.kl = f.kl + mc_kl_term(x.x, L, lp.x);
      f.kl = f.kl + mc_kl_term(x.y, L, lp.y);
      f.kl = f.kl + mc_kl_term(x.z, L, lp.z);
      f.kl = f.kl + mc_kl_term(x.w, L, lp.w);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    McFold b;
    b.h = __shfl_xor(f.h, o, 64);
    b.kl = __shfl_xor(f.kl, o, 64);
    b.mx = __shfl_xor(f.mx, o, 64);
    b.am = __shfl_xor(f.am, o, 64);
    b.cnt = __shfl_xor(f.cnt, o, 64);
    mc_fold_merge(f, b);
  }
  if (lane == 0) red_f[w] = f;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < LP_WAVES; ++k) mc_fold_merge(f, red_f[k]);
  const bool b = bad != 0;
  if (p.bma_nll) p.bma_nll[row] = (b || !has_t) ? NAN : -logf(pt);
  if (p.h_pred) p.h_pred[row] = b ? NAN : f.h;
  if (p.mi) p.mi[row] = b ? NAN : f.kl * inv_s;
  if (p.conf) p.conf[row] = b ? NAN : f.mx;
  if (p.pred) p.pred[row] = b ? -1 : f.am;
  if (p.rank) p.rank[row] = (b || !has_t) ? -1 : f.cnt;
}

}  // namespace
}  // namespace blm

extern "C" int blm_laplace_curvature(const float* logits, int64_t ld, float* a, int64_t lda, int rows, int V, void* stream) {
  if (!logits || !a) return blm_fail(BLM_ERR_INVALID, "blm_laplace_curvature: null operand");
  if (rows < 0 || V <= 0 || ld < V || lda < V || !blm::extents_ok({rows, (long)ld}) || !blm::extents_ok({rows, (long)lda}))
    return blm_fail(BLM_ERR_INVALID, "blm_laplace_curvature: bad shape (rows %d, V %d, ld %lld, lda %lld)", rows, V, (long long)ld,
                    (long long)lda);
  if (rows == 0) return BLM_OK;
  if (!(a == logits && lda == ld) && blm::overlaps(blm::span_of(logits, rows, ld, V), blm::span_of(a, rows, lda, V)))
    return blm_fail(BLM_ERR_INVALID, "blm_laplace_curvature: logits and a overlap (in place takes a == logits and lda == ld)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = ((ld | lda) & 3) == 0 && blm::aligned16(logits, a);
  if (vec && V <= 4096 * 3)
    hipLaunchKernelGGL(blm::curv_row_kernel<3>, dim3(rows), dim3(1024), 0, st, logits, (long)ld, a, (long)lda, V);
  else if (vec && V <= 4096 * 9)
    hipLaunchKernelGGL(blm::curv_row_kernel<9>, dim3(rows), dim3(1024), 0, st, logits, (long)ld, a, (long)lda, V);
  else
    hipLaunchKernelGGL(blm::curv_sweep_kernel, dim3(rows), dim3(1024), 0, st, logits, (long)ld, a, (long)lda, V, vec ? 1 : 0);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_laplace_row_stats(const float* z, int64_t ldz, const float* var, int64_t ldv, const int64_t* tgt, int R, int V,
                                     int link, float* nll, float* conf, float* entropy, int32_t* pred, int32_t* rank, float* vbar,
                                     void* stream) {
  if (!z || !var) return blm_fail(BLM_ERR_INVALID, "blm_laplace_row_stats: null operand");
  if (link != blm::LINK_PROBIT && link != blm::LINK_EXPEXP)
    return blm_fail(BLM_ERR_INVALID, "blm_laplace_row_stats: link %d is neither 0 (probit) nor 1 (expexp)", link);
  if (R < 0 || V <= 0 || ldz < V || ldv < V) return blm_fail(BLM_ERR_INVALID, "blm_laplace_row_stats: bad shape");
  if (!tgt && (nll || rank)) return blm_fail(BLM_ERR_INVALID, "blm_laplace_row_stats: nll and rank need targets");
  if (!blm::extents_ok({R, (long)ldz}) || !blm::extents_ok({R, (long)ldv}))
    return blm_fail(BLM_ERR_INVALID, "blm_laplace_row_stats: extents too large");
  if (R == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int vec = ((ldz | ldv) & 3) == 0 && blm::aligned16(z, var) ? 1 : 0;
  if (link == blm::LINK_PROBIT)
    hipLaunchKernelGGL(blm::laplace_row_stats_kernel<blm::LINK_PROBIT>, dim3(R), dim3(blm::LP_TPB), 0, st, z, (long)ldz, var,
                       (long)ldv, tgt, V, vec, nll, conf, entropy, pred, rank, vbar);
  else
    hipLaunchKernelGGL(blm::laplace_row_stats_kernel<blm::LINK_EXPEXP>, dim3(R), dim3(blm::LP_TPB), 0, st, z, (long)ldz, var,
                       (long)ldv, tgt, V, vec, nll, conf, entropy, pred, rank, vbar);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_laplace_mc_rows(const float* z, int64_t ldz, const float* var, int64_t ldv, const int64_t* tgt, int R, int V,
                                   int S, const blm_rng* rng, int64_t row0, float* bma_nll, float* nll_s, float* h_pred, float* mi,
                                   float* conf, int32_t* pred, int32_t* rank, void* stream) {
  if (!z || !var || !rng) return blm_fail(BLM_ERR_INVALID, "blm_laplace_mc_rows: null operand");
  if (S < 1 || S > BLM_LAPLACE_SAMPLES_MAX)
    return blm_fail(BLM_ERR_INVALID, "blm_laplace_mc_rows: S = %d outside 1..%d", S, BLM_LAPLACE_SAMPLES_MAX);
  if (R < 0 || V <= 0 || ldz < V || ldv < V) return blm_fail(BLM_ERR_INVALID, "blm_laplace_mc_rows: bad shape");
  if (row0 < 0 || row0 > blm::kMaxElems)
    return blm_fail(BLM_ERR_INVALID, "blm_laplace_mc_rows: row0 = %lld outside 0..2^40", (long long)row0);
  if (!tgt && (bma_nll || nll_s || rank)) return blm_fail(BLM_ERR_INVALID, "blm_laplace_mc_rows: bma_nll, nll_s and rank need targets");
  if (!blm::extents_ok({R, (long)ldz}) || !blm::extents_ok({R, (long)ldv}) || !blm::extents_ok({R, (long)BLM_LAPLACE_SAMPLES_MAX}))
    return blm_fail(BLM_ERR_INVALID, "blm_laplace_mc_rows: extents too large");
  if (R == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  blm::McArgs p;
  p.z = z, p.ldz = (long)ldz, p.var = var, p.ldv = (long)ldv, p.tgt = tgt;
  p.R = R, p.V = V, p.S = S;
  p.vec = ((ldz | ldv) & 3) == 0 && blm::aligned16(z, var) ? 1 : 0;
  p.seed = rng->seed, p.stream = rng->stream, p.row0 = (long)row0;
  p.bma_nll = bma_nll, p.nll_s = nll_s, p.h_pred = h_pred, p.mi = mi, p.conf = conf, p.pred = pred, p.rank = rank;
  hipLaunchKernelGGL(blm::laplace_mc_rows_kernel, dim3(R), dim3(blm::LP_TPB), 0, st, p);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
