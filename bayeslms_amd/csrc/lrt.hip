// Local reparameterisation of a variational linear layer (Kingma, Salimans & Welling 2015): the elementwise passes around the
// GEMM family's products.  The layer's pre-activations are sampled instead of its weights,
//   m = x mu^T,  v = x^2 (sigma^2)^T,  s = sqrt(v),  y = m + s * zeta,   zeta ~ N(0,1) per (row, column),
// so every row of the batch sees noise of its own.  No reference counterpart (the reference draws one W per step,
// model.py:1083-1107).  All four kernels are HBM-bound streams: 16-byte accesses where the operands allow them, a guarded
// scalar loop otherwise; no reductions, so nothing here depends on the deterministic mode.
//
// zeta is keyed like the dropout masks (blm_dropkey.h): element (row, col_offset + b, n) of a (rows, global_cols, N) tensor,
// four values per Philox block, so a data-parallel rank draws the columns of the one-process run and backward regenerates
// what forward drew.
#include "blm_device.h"
#include "blm_host.h"

namespace blm {

constexpr int TPB = 256;

static int grid_for(long items) {
  long g = (items + TPB - 1) / TPB;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}


struct ZetaKey {
  blm_rng rng;
  const float* zeta;  // handed in (M x N, local layout) or NULL: Philox
  int B, N, col_offset, global_cols;
};

// Global stream index of local flat element o = (row * B + b) * N + n.
__device__ __forceinline__ uint64_t zeta_index(const ZetaKey& k, long o) {
  if (k.global_cols == k.B) return (uint64_t)o;  // col_offset is 0 then
  const long m = o / k.N, n = o - m * k.N;
  const long row = m / k.B, b = m - row * k.B;
  return ((uint64_t)row * (uint64_t)k.global_cols + (uint64_t)(k.col_offset + b)) * (uint64_t)k.N + (uint64_t)n;
}
// N % 4 == 0 and o % 4 == 0: the four values are one Philox block.
__device__ __forceinline__ float4 zeta4(const ZetaKey& k, long o) {
  if (k.zeta) return *reinterpret_cast<const float4*>(k.zeta + o);
  return philox_normal4(k.rng, zeta_index(k, o) >> 2);
}
__device__ __forceinline__ float zeta1(const ZetaKey& k, long o) {
  if (k.zeta) return k.zeta[o];
  const uint64_t g = zeta_index(k, o);
  const float4 z = philox_normal4(k.rng, g >> 2);
  const int c = (int)(g & 3);
  return c == 0 ? z.x : (c == 1 ? z.y : (c == 2 ? z.z : z.w));
}

// mode 0: dst = src^2;  mode 1: dst = exp(2 src)
__global__ __launch_bounds__(TPB) void lrt_prepare_kernel(const float* __restrict__ src, float* __restrict__ dst, long n, int mode,
                                                          bool vec) {
  const long stride = (long)gridDim.x * TPB, t = (long)blockIdx.x * TPB + threadIdx.x;
  const long n4 = vec ? n >> 2 : 0;
  for (long i = t; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4*>(src)[i];
    float4 r;
    if (mode == 0) r = make_float4(a.x * a.x, a.y * a.y, a.z * a.z, a.w * a.w);
    else r = make_float4(__expf(2.f * a.x), __expf(2.f * a.y), __expf(2.f * a.z), __expf(2.f * a.w));
    reinterpret_cast<float4*>(dst)[i] = r;
  }
  for (long i = (n4 << 2) + t; i < n; i += stride) dst[i] = mode == 0 ? src[i] * src[i] : __expf(2.f * src[i]);
}

// y holds m and receives y; s holds v and receives sqrt(v).
__global__ __launch_bounds__(TPB) void lrt_combine_kernel(float* __restrict__ y, float* __restrict__ s, long n, ZetaKey k, bool vec) {
  const long stride = (long)gridDim.x * TPB, t = (long)blockIdx.x * TPB + threadIdx.x;
  if (vec) {
    for (long i = t; i < (n >> 2); i += stride) {
      const long o = i << 2;
      float4 m = *reinterpret_cast<const float4*>(y + o);
      const float4 v = *reinterpret_cast<const float4*>(s + o);
      const float4 z = zeta4(k, o);
      const float4 sd = make_float4(__builtin_sqrtf(v.x), __builtin_sqrtf(v.y), __builtin_sqrtf(v.z), __builtin_sqrtf(v.w));
      m.x = fmaf(sd.x, z.x, m.x); m.y = fmaf(sd.y, z.y, m.y); m.z = fmaf(sd.z, z.z, m.z); m.w = fmaf(sd.w, z.w, m.w);
      *reinterpret_cast<float4*>(y + o) = m;
      *reinterpret_cast<float4*>(s + o) = sd;
    }
  } else {
    for (long o = t; o < n; o += stride) {
      const float sd = __builtin_sqrtf(s[o]);
      y[o] = fmaf(sd, zeta1(k, o), y[o]);
      s[o] = sd;
    }
  }
}

// q = dy * zeta / (2 s), and 0 where s == 0 (a zero input row or sigma = 0: y = m there, no gradient through s)
__device__ __forceinline__ float lrt_q(float dy, float z, float s) { return s > 0.f ? 0.5f * dy * z / s : 0.f; }

__global__ __launch_bounds__(TPB) void lrt_bwd_factor_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                             float* __restrict__ q, long n, ZetaKey k, bool vec) {
  const long stride = (long)gridDim.x * TPB, t = (long)blockIdx.x * TPB + threadIdx.x;
  if (vec) {
    for (long i = t; i < (n >> 2); i += stride) {
      const long o = i << 2;
      const float4 g = *reinterpret_cast<const float4*>(dy + o);
      const float4 sd = *reinterpret_cast<const float4*>(s + o);
      const float4 z = zeta4(k, o);
      *reinterpret_cast<float4*>(q + o) = make_float4(lrt_q(g.x, z.x, sd.x), lrt_q(g.y, z.y, sd.y), lrt_q(g.z, z.z, sd.z), lrt_q(g.w, z.w, sd.w));
    }
  } else {
    for (long o = t; o < n; o += stride) q[o] = lrt_q(dy[o], zeta1(k, o), s[o]);
  }
}

// out = (acc ? out : 0) + scale * a * b; out may be a or b
__global__ __launch_bounds__(TPB) void lrt_mul_kernel(float* out, const float* a, const float* b, long n, float scale, bool acc, bool vec) {
  const long stride = (long)gridDim.x * TPB, t = (long)blockIdx.x * TPB + threadIdx.x;
  const long n4 = vec ? n >> 2 : 0;
  for (long i = t; i < n4; i += stride) {
    const float4 x = reinterpret_cast<const float4*>(a)[i], w = reinterpret_cast<const float4*>(b)[i];
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (acc) r = reinterpret_cast<const float4*>(out)[i];
    r.x += scale * x.x * w.x; r.y += scale * x.y * w.y; r.z += scale * x.z * w.z; r.w += scale * x.w * w.w;
    reinterpret_cast<float4*>(out)[i] = r;
  }
  for (long i = (n4 << 2) + t; i < n; i += stride) out[i] = (acc ? out[i] : 0.f) + scale * a[i] * b[i];
}

static bool make_zeta_key(ZetaKey& k, const float* zeta, const blm_rng* rng, int rows, int B, int N, int col_offset, int global_cols) {
  if ((!zeta && !rng) || col_offset < 0 || global_cols < 0 || !extents_ok({rows, B, N})) return false;
  const long gc = global_cols > 0 ? global_cols : B;
  if ((long)col_offset + B > gc || !extents_ok({rows, gc, N})) return false;
  k = ZetaKey{};
  if (rng) k.rng = *rng;
  k.zeta = zeta;
  k.B = B; k.N = N; k.col_offset = col_offset; k.global_cols = (int)gc;
  return true;
}

}  // namespace blm

using namespace blm;
#define ST static_cast<hipStream_t>(stream)

extern "C" int blm_lrt_prepare(const float* src, float* dst, int64_t n, int mode, void* stream) {
  if (!src || !dst || n < 0 || n > kMaxElems || (mode != 0 && mode != 1)) return blm_fail(BLM_ERR_INVALID, "blm_lrt_prepare: bad arguments");
  if (n == 0) return BLM_OK;
  hipLaunchKernelGGL(lrt_prepare_kernel, dim3(grid_for(n / 4 + 1)), dim3(TPB), 0, ST, src, dst, (long)n, mode, aligned16(src, dst));
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_lrt_combine(float* y, float* s, const float* zeta, const blm_rng* rng, int rows, int B, int N, int col_offset,
                               int global_cols, void* stream) {
  ZetaKey k;
  if (!y || !s || y == s || !make_zeta_key(k, zeta, rng, rows, B, N, col_offset, global_cols))
    return blm_fail(BLM_ERR_INVALID, "blm_lrt_combine: bad arguments");
  const long n = (long)rows * B * N;
  if (n == 0) return BLM_OK;
  const bool vec = N % 4 == 0 && aligned16(y, s, zeta);
  hipLaunchKernelGGL(lrt_combine_kernel, dim3(grid_for(vec ? n / 4 : n)), dim3(TPB), 0, ST, y, s, n, k, vec);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_lrt_bwd_factor(const float* dy, const float* s, float* q, const float* zeta, const blm_rng* rng, int rows, int B,
                                  int N, int col_offset, int global_cols, void* stream) {
  ZetaKey k;
  if (!dy || !s || !q || !make_zeta_key(k, zeta, rng, rows, B, N, col_offset, global_cols))
    return blm_fail(BLM_ERR_INVALID, "blm_lrt_bwd_factor: bad arguments");
  const long n = (long)rows * B * N;
  if (n == 0) return BLM_OK;
  const bool vec = N % 4 == 0 && aligned16(dy, s, q, zeta);
  hipLaunchKernelGGL(lrt_bwd_factor_kernel, dim3(grid_for(vec ? n / 4 : n)), dim3(TPB), 0, ST, dy, s, q, n, k, vec);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_lrt_mul(float* out, const float* a, const float* b, int64_t n, float scale, int accumulate, void* stream) {
  if (!out || !a || !b || n < 0 || n > kMaxElems) return blm_fail(BLM_ERR_INVALID, "blm_lrt_mul: bad arguments");
  if (n == 0) return BLM_OK;
  hipLaunchKernelGGL(lrt_mul_kernel, dim3(grid_for(n / 4 + 1)), dim3(TPB), 0, ST, out, a, b, (long)n, scale, accumulate != 0,
                     aligned16(out, a, b));
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
