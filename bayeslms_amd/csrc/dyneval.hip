// Dynamic evaluation (Krause, Kahembwe, Murray, Renals, ICML 2018): the per-window update of every weight, pulled back towards
// the trained weights, and the gradient statistics that scale it.  Definitions: include/bayeslm.h.
//
//   blm_dyneval_accum    ms[i] += g[i]^2                                              (3 streams of n floats)
//   blm_dyneval_rms      rms[i] = sqrt(ms[i] / count); mean = { mean of rms over ms > 0, number of those }
//   blm_dyneval_update   p[i] = p[i] - step + d (p0[i] - p[i]), g[i] = 0 on request   (5 streams sgd, 6 rms)
//
// All three are memory-bound streaming kernels: one grid-stride pass of 16-byte loads and stores over the aligned body and a
// scalar tail, a grid of at most DYN_GRID workgroups of 256 lanes (the single-tensor grid of clip_sgd_multi_kernel).  Pointers
// that are not 16-byte aligned are accepted: the whole array then takes the scalar path, as in clip_sgd_multi_kernel.
// The mean is summed in double in two stages, each in a fixed order, without atomics: the same bits in every run.
#include <cmath>

#include "blm_device.h"
#include "blm_host.h"

namespace blm {
namespace {

constexpr int DYN_TPB = 256;
constexpr int DYN_GRID = 2048;
constexpr int DYN_RMS_GRID = BLM_DYNEVAL_RMS_WS_FLOATS / 4;  // two doubles per workgroup

inline int dyn_grid(long n, int cap) {
  const long blocks = (n / 4 + DYN_TPB - 1) / DYN_TPB;  // one float4 per lane and trip
  return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

__global__ __launch_bounds__(DYN_TPB) void dyneval_accum_kernel(float* __restrict__ ms, const float* __restrict__ g, long n) {
  const long n4 = aligned16(ms, g) ? (n >> 2) : 0;
  const long stride = (long)gridDim.x * DYN_TPB, first = (long)blockIdx.x * DYN_TPB + threadIdx.x;
  for (long i = first; i < n4; i += stride) {
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(ms)[i];
    mv.x += gv.x * gv.x; mv.y += gv.y * gv.y; mv.z += gv.z * gv.z; mv.w += gv.w * gv.w;
    reinterpret_cast<float4*>(ms)[i] = mv;
  }
  for (long i = (n4 << 2) + first; i < n; i += stride) ms[i] += g[i] * g[i];
}

// the two sums of a workgroup, lane order then wave order: fixed
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[2]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w][0] = a, red[w][1] = b;
  __syncthreads();
  a = 0.0, b = 0.0;
#pragma unroll
  for (int i = 0; i < DYN_TPB / 64; ++i) a += red[i][0], b += red[i][1];
}

__device__ __forceinline__ float rms_of(float ms, float count, double& sum, double& live) {
  const float r = sqrtf(ms / count);
  if (ms > 0.f) sum += (double)r, live += 1.0;
  return r;
}

// stage 1: rms and each workgroup's (sum of live rms, number of live entries) -> part[2 * blockIdx.x ..]
__global__ __launch_bounds__(DYN_TPB) void dyneval_rms_kernel(const float* __restrict__ ms, float* __restrict__ rms, long n,
                                                              float count, double* __restrict__ part) {
  __shared__ double red[DYN_TPB / 64][2];
  double sum = 0.0, live = 0.0;
  const long n4 = aligned16(ms, rms) ? (n >> 2) : 0;
  const long stride = (long)gridDim.x * DYN_TPB, first = (long)blockIdx.x * DYN_TPB + threadIdx.x;
  for (long i = first; i < n4; i += stride) {
    const float4 mv = reinterpret_cast<const float4*>(ms)[i];
    float4 rv;
    rv.x = rms_of(mv.x, count, sum, live); rv.y = rms_of(mv.y, count, sum, live);
    rv.z = rms_of(mv.z, count, sum, live); rv.w = rms_of(mv.w, count, sum, live);
    reinterpret_cast<float4*>(rms)[i] = rv;
  }
  for (long i = (n4 << 2) + first; i < n; i += stride) rms[i] = rms_of(ms[i], count, sum, live);
  block_sum2(sum, live, red);
  if (threadIdx.x == 0) part[2 * blockIdx.x] = sum, part[2 * blockIdx.x + 1] = live;
}

// stage 2, one workgroup: lane t adds the partials t, t + 256, ... in that order, then the workgroup's sum as above
__global__ __launch_bounds__(DYN_TPB) void dyneval_mean_kernel(const double* __restrict__ part, int parts, float* __restrict__ mean) {
  __shared__ double red[DYN_TPB / 64][2];
  double sum = 0.0, live = 0.0;
  for (int i = threadIdx.x; i < parts; i += DYN_TPB) sum += part[2 * i], live += part[2 * i + 1];
  block_sum2(sum, live, red);
  if (threadIdx.x == 0) {
    mean[0] = live > 0.0 ? (float)(sum / live) : 0.f;
    mean[1] = (float)live;
  }
}

struct DynScale {
  float lr, decay, eps_rbar, decay_over_rbar;  // the last two: eps * rbar and decay / rbar, rounded once (rms rule)
};

// fp32, in exactly this order and without contraction: p - step + d * (p0 - p)
template <bool RMS>
__device__ __forceinline__ float dyn_one(float p, float g, float p0, float r, const DynScale& s) {
#pragma clang fp contract(off)
  float step = s.lr * g, d = s.decay;
  if (RMS) {
    step = g == 0.f ? 0.f : step / (r + s.eps_rbar);  // g = 0 does not move, whatever the denominator
    d = s.decay_over_rbar * r;
  }
  d = fminf(1.0f, d);
  return p - step + d * (p0 - p);
}

template <bool RMS, bool ZERO>
__global__ __launch_bounds__(DYN_TPB) void dyneval_update_kernel(float* __restrict__ p, float* __restrict__ g,
                                                                 const float* __restrict__ p0, const float* __restrict__ rms,
                                                                 const float* __restrict__ mean, long n, float lr, float decay,
                                                                 float eps) {
#pragma clang fp contract(off)
  DynScale s = {lr, decay, 0.f, 0.f};
  if (RMS) {
    const float rbar = mean[0];
    s.eps_rbar = eps * rbar;
    s.decay_over_rbar = decay / rbar;
  }
  const long n4 = aligned16(p, g, p0, rms) ? (n >> 2) : 0;
  const long stride = (long)gridDim.x * DYN_TPB, first = (long)blockIdx.x * DYN_TPB + threadIdx.x;
  for (long i = first; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    const float4 qv = reinterpret_cast<const float4*>(p0)[i];
    float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (RMS) rv = reinterpret_cast<const float4*>(rms)[i];
    pv.x = dyn_one<RMS>(pv.x, gv.x, qv.x, rv.x, s); pv.y = dyn_one<RMS>(pv.y, gv.y, qv.y, rv.y, s);
    pv.z = dyn_one<RMS>(pv.z, gv.z, qv.z, rv.z, s); pv.w = dyn_one<RMS>(pv.w, gv.w, qv.w, rv.w, s);
    reinterpret_cast<float4*>(p)[i] = pv;
    if (ZERO) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (long i = (n4 << 2) + first; i < n; i += stride) {
    p[i] = dyn_one<RMS>(p[i], g[i], p0[i], RMS ? rms[i] : 0.f, s);
    if (ZERO) g[i] = 0.f;
  }
}

inline bool finite_nonneg(float v) { return v >= 0.f && v <= 3.402823466e38f; }

}  // namespace
}  // namespace blm

extern "C" int blm_dyneval_accum(float* ms, const float* g, int64_t n, void* stream) {
  if (!ms || !g) return blm_fail(BLM_ERR_INVALID, "blm_dyneval_accum: null operand");
  if (n < 0 || n > blm::kMaxElems) return blm_fail(BLM_ERR_INVALID, "blm_dyneval_accum: n = %lld outside 0..2^40", (long long)n);
  if (n == 0) return BLM_OK;
  hipLaunchKernelGGL(blm::dyneval_accum_kernel, dim3(blm::dyn_grid((long)n, blm::DYN_GRID)), dim3(blm::DYN_TPB), 0,
                     static_cast<hipStream_t>(stream), ms, g, (long)n);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_dyneval_rms(const float* ms, int64_t n, int count, float* rms, float* mean, float* ws, void* stream) {
  if (!ms || !rms || !mean || !ws) return blm_fail(BLM_ERR_INVALID, "blm_dyneval_rms: null operand");
  if (n < 0 || n > blm::kMaxElems) return blm_fail(BLM_ERR_INVALID, "blm_dyneval_rms: n = %lld outside 0..2^40", (long long)n);
  if (count < 1) return blm_fail(BLM_ERR_INVALID, "blm_dyneval_rms: count %d < 1", count);
  if (reinterpret_cast<uintptr_t>(ws) & 7)
    return blm_fail(BLM_ERR_INVALID, "blm_dyneval_rms: ws holds doubles and must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(ws);
  int parts = 0;
  if (n > 0) {
    parts = blm::dyn_grid((long)n, blm::DYN_RMS_GRID);
    hipLaunchKernelGGL(blm::dyneval_rms_kernel, dim3(parts), dim3(blm::DYN_TPB), 0, st, ms, rms, (long)n, (float)count, part);
    BLM_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(blm::dyneval_mean_kernel, dim3(1), dim3(blm::DYN_TPB), 0, st, part, parts, mean);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_dyneval_update(float* p, float* g, const float* p0, const float* rms, const float* mean, int64_t n, float lr,
                                  float decay, float eps, int zero_grad, void* stream) {
  if (!p || !g || !p0) return blm_fail(BLM_ERR_INVALID, "blm_dyneval_update: null operand");
  if ((rms == nullptr) != (mean == nullptr))
    return blm_fail(BLM_ERR_INVALID, "blm_dyneval_update: rms and mean go together (both for the rms rule, neither for sgd)");
  if (n < 0 || n > blm::kMaxElems) return blm_fail(BLM_ERR_INVALID, "blm_dyneval_update: n = %lld outside 0..2^40", (long long)n);
  if (!blm::finite_nonneg(lr) || !blm::finite_nonneg(decay) || !blm::finite_nonneg(eps))
    return blm_fail(BLM_ERR_INVALID, "blm_dyneval_update: lr %g, decay %g, eps %g: each must be finite and >= 0", (double)lr,
                    (double)decay, (double)eps);
  if (n == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(blm::dyn_grid((long)n, blm::DYN_GRID)), block(blm::DYN_TPB);
  const long nn = (long)n;
  if (rms) {
    if (zero_grad) hipLaunchKernelGGL((blm::dyneval_update_kernel<true, true>), grid, block, 0, st, p, g, p0, rms, mean, nn, lr, decay, eps);
    else hipLaunchKernelGGL((blm::dyneval_update_kernel<true, false>), grid, block, 0, st, p, g, p0, rms, mean, nn, lr, decay, eps);
  } else {
    if (zero_grad) hipLaunchKernelGGL((blm::dyneval_update_kernel<false, true>), grid, block, 0, st, p, g, p0, rms, mean, nn, lr, decay, eps);
    else hipLaunchKernelGGL((blm::dyneval_update_kernel<false, false>), grid, block, 0, st, p, g, p0, rms, mean, nn, lr, decay, eps);
  }
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
