// Continuous neural cache (Grave, Joulin, Usunier, ICLR 2017): banded Q K^T on the f32 matrix cores
// (v_mfma_f32_32x32x2_f32) whose scores are reduced on the fly to two log-sums per query and theta; no score reaches memory.
//
//   lse[j][m]   = log sum_{i in R_m}                     exp(theta_j q_m . k_i)
//   match[j][m] = log sum_{i in R_m, label[i] == tgt[m]} exp(theta_j q_m . k_i)
//   R_m = [max(lo[m], hi[m] - window, 0), min(hi[m], Nk))          (-inf over an empty set)
//
// Design: a workgroup of 4 waves owns 128 consecutive queries, one MFMA column tile of 32 queries per wave, and walks key tiles
// of 128 rows over [min start, max end) of its queries' ranges -- for the evaluation's band hi[m] = m that is window + 128
// keys, whatever Nk is.  Both operands are k-contiguous, so both go global -> registers -> LDS as tile[row][KS] images
// (gemm_f32_mfma.h: r2s_kmaj; the K tail and unaligned operands through its guarded loader g2r_kmaj, any K, any alignment);
// the next K step's loads are in flight while the current one is multiplied.  The score tile is computed TRANSPOSED,
// S^T[key][query] = K Q^T (attention_mfma.hip): the MFMA result then has ONE QUERY PER LANE and its 4 x 16 keys in the
// accumulator registers, so the masked online log-sum-exp is register arithmetic, a wave skips the 32-key sub-tiles that miss the
// ranges of its own 32 queries, and the two lane halves of a query meet in ONE shuffle at the very end.
//
// Arithmetic: theta >= 0, so the running maximum mx of the RAW score serves every theta_j; per theta two sums relative to it,
// all keys and matching keys: e = exp2(theta_j log2(e) (s - mx)).  lse = theta_j mx + log(sum).  A matching key whose weight
// underflows float32 beside the window's maximum (theta (mx - s) > 87) leaves match at -inf: a cache probability below 1e-38.
// No atomics, one fixed order of every sum: the same bits in every run, deterministic mode or not.
#include <cmath>

#include "gemm_f32_mfma.h"

namespace blm {
namespace {

constexpr int CQ = 128;  // queries and keys per tile (4 MFMA tiles of 32)

template <int J>
struct CacheThetas {
  float theta[J];
  float t2[J];  // theta * log2(e)
};

struct CacheP {
  const float* q; long ldq;
  const float* k; long ldk;
  const int64_t* label;
  const int64_t* tgt;
  const int32_t* lo;
  const int32_t* hi;
  int window, M, Nk, K;
  int vq, vk;  // float4 loads allowed (16-byte aligned base, ld % 4 == 0)
  float* lse;
  float* match;
};

// MFMA row index held in accumulator register r by a lane of half h
__device__ __forceinline__ constexpr int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// two workgroups per CU (second launch bound: waves per SIMD): 254..256 VGPRs, nothing spilled, so one workgroup's loads and
// LDS round trip run behind the other's MFMAs
template <int J>
__global__ __launch_bounds__(256, 2) void cache_scores_kernel(const CacheP p, const CacheThetas<J> th, int count) {
  __shared__ __attribute__((aligned(16))) float Qs[CQ * KS];
  __shared__ __attribute__((aligned(16))) float Ks[CQ * KS];
  __shared__ long long labs[CQ];
  __shared__ int wrange[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * CQ;
  const int m = m0 + 32 * wave + li;
  const bool mok = m < p.M;

  // the query's clamped key range [st, en): whatever lo / hi hold, 0 <= st, en <= Nk
  int st = 0, en = 0;
  long long tgt = 0;
  if (mok) {
    const long long h = p.hi[m], l = p.lo ? (long long)p.lo[m] : 0;
    long long s = h - (long long)p.window;
    s = s > l ? s : l;
    s = s > 0 ? s : 0;
    long long e = h < (long long)p.Nk ? h : (long long)p.Nk;
    e = e > 0 ? e : 0;
    s = s < (long long)p.Nk ? s : (long long)p.Nk;
    st = (int)s;
    en = (int)e;
    tgt = p.tgt[m];
  }
  // the wave's and the workgroup's hull of the non-empty ranges
  int wlo = st < en ? st : 0x7fffffff, whi = st < en ? en : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wlo = min(wlo, __shfl_xor(wlo, o, 64));
    whi = max(whi, __shfl_xor(whi, o, 64));
  }
  if (lane == 0) { wrange[2 * wave] = wlo; wrange[2 * wave + 1] = whi; }
  __syncthreads();
  const int blo = __builtin_amdgcn_readfirstlane(min(min(wrange[0], wrange[2]), min(wrange[4], wrange[6])));
  const int bhi = __builtin_amdgcn_readfirstlane(max(max(wrange[1], wrange[3]), max(wrange[5], wrange[7])));
  wlo = __builtin_amdgcn_readfirstlane(wlo);
  whi = __builtin_amdgcn_readfirstlane(whi);

  float mx = -INFINITY;
  float sl[J], sm[J];
#pragma unroll
  for (int j = 0; j < J; ++j) sl[j] = sm[j] = 0.f;

  const int nkc = (p.K + BK - 1) / BK;
  const int ntile = blo < bhi ? (bhi - blo + CQ - 1) / CQ : 0;
  if (ntile > 0) {
    float4 rq[CQ / 32], rk[CQ / 32];
    long long rl = 0;
    // A tile of 128 rows x one whole K step inside a 16-byte aligned operand is loaded without a branch, its four rows per thread
    // a uniform 32 ld apart; only tiles across the end of an operand, the K tail and unaligned operands take the guarded loader,
    // whose per-element branches drain the loads in flight.
    auto rows32 = [&](const float* src, long ld, int row0, int rows, int k0, bool vec, float4(&r)[CQ / 32]) {
      if (vec && k0 + BK <= p.K && row0 + CQ <= rows) {
        const float* base = src + (long)(row0 + (tid >> 3)) * ld + k0 + 4 * (tid & 7);
#pragma unroll
        for (int j = 0; j < CQ / 32; ++j) r[j] = *reinterpret_cast<const float4*>(base + 32 * j * ld);
      } else {
        g2r_kmaj<CQ>(src, ld, row0, rows, k0, p.K, vec, r);
      }
    };
    auto fetch = [&](int it, int kc) {
      const int kb = blo + CQ * it;
      rows32(p.q, p.ldq, m0, p.M, kc * BK, p.vq != 0, rq);
      rows32(p.k, p.ldk, kb, p.Nk, kc * BK, p.vk != 0, rk);
      if (kc == 0 && tid < CQ) rl = p.label[min(kb + tid, p.Nk - 1)];  // a key >= Nk is in no range
    };
    fetch(0, 0);
    const float* qrow = Qs + (32 * wave + li) * KS + 4 * lh;
    const float* krow = Ks + li * KS + 4 * lh;
#pragma unroll 1
    for (int it = 0; it < ntile; ++it) {
      const int kb = blo + CQ * it;
      // 32-key sub-tiles that meet the hull of this wave's ranges (wave-uniform)
      bool need[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) need[i] = kb + 32 * i < whi && kb + 32 * i + 32 > wlo;
      f32x16 acc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = (f32x16)(0.f);
#pragma unroll 1
      for (int kc = 0; kc < nkc; ++kc) {
        __syncthreads();  // the previous step's fragment reads (and the previous tile's label reads) are done
        r2s_kmaj<CQ>(Qs, rq);
        r2s_kmaj<CQ>(Ks, rk);
        if (kc == 0 && tid < CQ) labs[tid] = rl;
        __syncthreads();
        if (kc + 1 < nkc) fetch(it, kc + 1);
        else if (it + 1 < ntile) fetch(it + 1, 0);
        // k order inside the step: k(t, s, half) = 8t + 4 half + s for both operands -> one 16-byte LDS read per group t
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (need[i]) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const float4 a = *reinterpret_cast<const float4*>(krow + 32 * i * KS + 8 * t);
              const float4 b = *reinterpret_cast<const float4*>(qrow + 8 * t);
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[i], 0, 0, 0);
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[i], 0, 0, 0);
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[i], 0, 0, 0);
              acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[i], 0, 0, 0);
            }
          }
        }
      }
      // ---- the tile's scores into the running sums: lane = query, registers = keys kb + 32 i + crow(r, lh)
      float tm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (need[i]) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kb + 32 * i + crow(r, lh);
            if (key >= st && key < en) tm = fmaxf(tm, acc[i][r]);
          }
        }
      }
      if (tm > mx) {
        if (mx > -INFINITY) {
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const float f = __builtin_amdgcn_exp2f(th.t2[j] * (mx - tm));
            sl[j] *= f;
            sm[j] *= f;
          }
        }
        mx = tm;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (need[i]) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kk = 32 * i + crow(r, lh);
            const int key = kb + kk;
            const bool ok = key >= st && key < en;
            const bool hit = ok && labs[kk] == tgt;
            const float d = ok ? acc[i][r] - mx : 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
              const float e = ok ? __builtin_amdgcn_exp2f(th.t2[j] * d) : 0.f;
              sl[j] += e;
              sm[j] += hit ? e : 0.f;
            }
          }
        }
      }
    }
  }
  // ---- the two lane halves of a query hold disjoint keys: one exchange, half 0 first
  {
    const float mo = __shfl_xor(mx, 32, 64);
    const float mm = fmaxf(mx, mo);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float f = mx > -INFINITY ? __builtin_amdgcn_exp2f(th.t2[j] * (mx - mm)) : 0.f;
      const float a = sl[j] * f, b = sm[j] * f;
      const float ao = __shfl_xor(a, 32, 64), bo = __shfl_xor(b, 32, 64);
      sl[j] = a + ao;
      sm[j] = b + bo;
    }
    mx = mm;
  }
  if (mok && lh == 0) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
      if (j >= count) break;
      const size_t o = (size_t)j * p.M + m;
      p.lse[o] = mx > -INFINITY ? __builtin_fmaf(th.theta[j], mx, logf(sl[j])) : -INFINITY;
      p.match[o] = sm[j] > 0.f ? __builtin_fmaf(th.theta[j], mx, logf(sm[j])) : -INFINITY;
    }
  }
}

template <int J>
void launch_cache(const CacheP& p, const blm_cache_thetas* t, hipStream_t st) {
  CacheThetas<J> th;
  for (int j = 0; j < J; ++j) {
    const float v = t->theta[j < t->count ? j : 0];  // a surplus slot repeats slot 0 and is never written
    th.theta[j] = v;
    th.t2[j] = (float)((double)v * 1.4426950408889634);
  }
  hipLaunchKernelGGL((cache_scores_kernel<J>), dim3((p.M + CQ - 1) / CQ), dim3(256), 0, st, p, th, (int)t->count);
}

}  // namespace
}  // namespace blm

extern "C" int blm_cache_scores(const float* q, int64_t ldq, const float* k, int64_t ldk, const int64_t* label, const int64_t* tgt,
                                const int32_t* lo, const int32_t* hi, int window, int M, int Nk, int K,
                                const blm_cache_thetas* thetas, float* lse, float* match, float* ws, void* stream) {
  (void)ws;  // no workspace: nothing leaves the registers but the two log-sums
  if (!q || !k || !label || !tgt || !hi || !thetas || !lse || !match)
    return blm_fail(BLM_ERR_INVALID, "blm_cache_scores: null operand");
  if (thetas->abi_version != BLM_ABI_VERSION)
    return blm_fail(BLM_ERR_ABI, "blm_cache_scores: blm_cache_thetas.abi_version %u, library %u", thetas->abi_version,
                    BLM_ABI_VERSION);
  if (thetas->count < 1 || thetas->count > BLM_CACHE_THETAS_MAX)
    return blm_fail(BLM_ERR_INVALID, "blm_cache_scores: count %d outside 1..%d", thetas->count, BLM_CACHE_THETAS_MAX);
  for (int j = 0; j < thetas->count; ++j)
    if (!(thetas->theta[j] >= 0.f) || !(thetas->theta[j] <= 3.402823466e38f))
      return blm_fail(BLM_ERR_INVALID, "blm_cache_scores: theta[%d] = %g is not a finite number >= 0", j, (double)thetas->theta[j]);
  if (M < 0 || Nk < 0 || K < 1 || ldq < K || ldk < K) return blm_fail(BLM_ERR_INVALID, "blm_cache_scores: bad shape");
  if (window < 1) return blm_fail(BLM_ERR_INVALID, "blm_cache_scores: window %d < 1", window);
  if (!blm::extents_ok({M, (long)ldq}) || !blm::extents_ok({Nk, (long)ldk}) || !blm::extents_ok({M, (long)BLM_CACHE_THETAS_MAX}) ||
      !blm::extents_ok({K}))
    return blm_fail(BLM_ERR_INVALID, "blm_cache_scores: extents too large");
  if (M == 0) return BLM_OK;
  blm::CacheP p;
  p.q = q, p.ldq = (long)ldq, p.k = k, p.ldk = (long)ldk;
  p.label = label, p.tgt = tgt, p.lo = lo, p.hi = hi;
  p.window = window, p.M = M, p.Nk = Nk, p.K = K;
  p.vq = blm::aligned16(q) && ldq % 4 == 0;
  p.vk = blm::aligned16(k) && ldk % 4 == 0;
  p.lse = lse, p.match = match;
  hipStream_t st = static_cast<hipStream_t>(stream);
  blm::for_slots(thetas->count, [&](auto J) { blm::launch_cache<J()>(p, thetas, st); });
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
