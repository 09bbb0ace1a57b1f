// Stochastic-gradient MCMC (Welling and Teh, ICML 2011; Li, Chen, Carlson, Carin, AAAI 2016; Gan, Li, Chen, Pu, Su, Carin,
// ACL 2017): one weight update of SGLD or preconditioned SGLD over a model held in one flat buffer.  Definitions:
// include/bayeslm.h.
//
//   blm_sgmcmc_update   sgld:  p = p - lr d + sigma xi                                  (3 streams of n floats)
//                       psgld: v = alpha v + (1 - alpha) d^2, G = 1 / (damping + sqrt(v)),
//                              p = p - lr G d + sigma sqrt(G) xi                        (5 streams)
//                       d = c g + weight_decay p, c the global-norm clip of blm_clip_sgd_multi
//
// A memory-bound streaming kernel in dyneval.hip's shape: one grid-stride pass of 16-byte loads and stores over the aligned
// body and a scalar tail, a grid of at most SGM_GRID workgroups of 256 lanes; pointers that are not 16-byte aligned take the
// scalar path for the whole array.  xi[i] is element i of the Philox normal stream of the blm_rng handed in, i the index into
// the array handed in: the body takes block i4 for its float4 i4, the scalar path and the tail component i & 3 of block
// i >> 2, so an element gets the same noise on either path.  Contraction is off, so it gets the same bits too.  sigma == 0
// launches a form without the generator.  The Gamma(theta) term of Li et al. (the derivative of the preconditioner) is
// dropped, as their practical algorithm drops it.  No atomics, no reductions: the same bits in every run.
#include <cmath>

#include "blm_device.h"
#include "blm_host.h"

namespace blm {
namespace {

constexpr int SGM_TPB = 256;
constexpr int SGM_GRID = 2048;

inline int sgm_grid(long n) {
  const long blocks = (n / 4 + SGM_TPB - 1) / SGM_TPB;  // one float4 per lane and trip
  return (int)(blocks < 1 ? 1 : (blocks > SGM_GRID ? SGM_GRID : blocks));
}

struct SgmCoef {
  float c, lr, wd, sigma, alpha, one_m_alpha, damping;
};

// fp32, in exactly this order and without contraction (include/bayeslm.h)
template <bool PRE, bool NOISE>
__device__ __forceinline__ void sgm_one(float& p, float g, float& v, float xi, const SgmCoef& s) {
#pragma clang fp contract(off)
  const float d = s.c * g + s.wd * p;
  if (PRE) {
    v = s.alpha * v + (s.one_m_alpha * d) * d;
    const float G = 1.0f / (s.damping + __builtin_sqrtf(v));
    p = p - (s.lr * G) * d;
    if (NOISE) p = p + (s.sigma * __builtin_sqrtf(G)) * xi;
  } else {
    p = p - s.lr * d;
    if (NOISE) p = p + s.sigma * xi;
  }
}

template <bool PRE, bool NOISE>
__global__ __launch_bounds__(SGM_TPB) void sgmcmc_update_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                float* __restrict__ v, const float* __restrict__ sq, long n,
                                                                float clip, float gs, SgmCoef s, blm_rng rng) {
#pragma clang fp contract(off)
  // gradients are gs * g: the norm of the scaled gradient, as in clip_sgd_multi_kernel
  const float norm = sqrtf(sq[0]) * gs;
  s.c = fminf(1.0f, clip / (norm + 1e-6f)) * gs;
  const long n4 = aligned16(p, g, v) ? (n >> 2) : 0;
  const long stride = (long)gridDim.x * SGM_TPB, first = (long)blockIdx.x * SGM_TPB + threadIdx.x;
  for (long i = first; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 vv = make_float4(0.f, 0.f, 0.f, 0.f), z = vv;
    if (PRE) vv = reinterpret_cast<float4*>(v)[i];
    if (NOISE) z = philox_normal4(rng, (uint64_t)i);
    sgm_one<PRE, NOISE>(pv.x, gv.x, vv.x, z.x, s); sgm_one<PRE, NOISE>(pv.y, gv.y, vv.y, z.y, s);
    sgm_one<PRE, NOISE>(pv.z, gv.z, vv.z, z.z, s); sgm_one<PRE, NOISE>(pv.w, gv.w, vv.w, z.w, s);
    reinterpret_cast<float4*>(p)[i] = pv;
    if (PRE) reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (long i = (n4 << 2) + first; i < n; i += stride) {
    float pv = p[i], vv = PRE ? v[i] : 0.f, xi = 0.f;
    if (NOISE) xi = comp(philox_normal4(rng, (uint64_t)i >> 2), (int)(i & 3));
    sgm_one<PRE, NOISE>(pv, g[i], vv, xi, s);
    p[i] = pv;
    if (PRE) v[i] = vv;
  }
}

inline bool sgm_finite_nonneg(float v) { return v >= 0.f && v <= 3.402823466e38f; }

}  // namespace
}  // namespace blm

extern "C" int blm_sgmcmc_update(float* p, const float* g, float* v, const float* sq, int64_t n, float clip, float lr,
                                 float grad_scale, float weight_decay, float sigma, float alpha, float damping, const blm_rng* rng,
                                 void* stream) {
  if (!p || !g || !sq) return blm_fail(BLM_ERR_INVALID, "blm_sgmcmc_update: null operand");
  if (n < 0 || n > blm::kMaxElems) return blm_fail(BLM_ERR_INVALID, "blm_sgmcmc_update: n = %lld outside 0..2^40", (long long)n);
  if (!(clip > 0.f)) return blm_fail(BLM_ERR_INVALID, "blm_sgmcmc_update: clip %g must be > 0", (double)clip);
  if (!blm::sgm_finite_nonneg(lr) || !blm::sgm_finite_nonneg(sigma) || !blm::sgm_finite_nonneg(weight_decay))
    return blm_fail(BLM_ERR_INVALID, "blm_sgmcmc_update: lr %g, sigma %g, weight_decay %g: each must be finite and >= 0", (double)lr,
                    (double)sigma, (double)weight_decay);
  if (v && (!(alpha >= 0.f && alpha < 1.f) || !(damping > 0.f)))
    return blm_fail(BLM_ERR_INVALID, "blm_sgmcmc_update: with v, alpha %g must lie in [0, 1) and damping %g be > 0", (double)alpha,
                    (double)damping);
  if (!rng && sigma > 0.f) return blm_fail(BLM_ERR_INVALID, "blm_sgmcmc_update: sigma %g > 0 without an rng", (double)sigma);
  if (n == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(blm::sgm_grid((long)n)), block(blm::SGM_TPB);
  const long nn = (long)n;
  const blm::SgmCoef s = {0.f, lr, weight_decay, sigma, alpha, 1.0f - alpha, damping};
  const blm_rng r = rng ? *rng : blm_rng{0, 0, 0};
  const bool noise = sigma > 0.f;
  if (v) {
    if (noise) hipLaunchKernelGGL((blm::sgmcmc_update_kernel<true, true>), grid, block, 0, st, p, g, v, sq, nn, clip, grad_scale, s, r);
    else hipLaunchKernelGGL((blm::sgmcmc_update_kernel<true, false>), grid, block, 0, st, p, g, v, sq, nn, clip, grad_scale, s, r);
  } else {
    if (noise) hipLaunchKernelGGL((blm::sgmcmc_update_kernel<false, true>), grid, block, 0, st, p, g, v, sq, nn, clip, grad_scale, s, r);
    else hipLaunchKernelGGL((blm::sgmcmc_update_kernel<false, false>), grid, block, 0, st, p, g, v, sq, nn, clip, grad_scale, s, r);
  }
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
