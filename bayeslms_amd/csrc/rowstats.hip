// Row statistics of a matrix of logits or log-probabilities (engine.evaluate_report): per row the target's NLL, the
// confidence (largest probability), the entropy, the prediction and the target's rank, from ONE read of the row.  Vector ALU,
// bound by the bytes it reads: one 256-thread workgroup per row, every lane carries an online softmax state (running max and its
// lowest index, sum of exp(x - max), sum of exp(x - max) (x - max), rank count) that is rescaled when its max moves, and the
// lanes' states are merged in a fixed order (xor butterfly inside a wave, then the four waves in turn through LDS): no atomics,
// the same bits in every run.
#include "blm_device.h"
#include "blm_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// s = sum exp(x - m), t = sum exp(x - m) (x - m) over the finite columns seen so far: log-sum-exp = m + log s and
// entropy = log s - t / s, both free of the cancellation that sum p x has for rows far from 0.
struct Acc {
  float m, s, t;
  int am, cnt, bad;
};

// the state re-expressed for a max M > a.m (a.m == -inf: nothing summed yet, s = t = 0 stay)
__device__ __forceinline__ void rescale(Acc& a, float M) {
  if (a.m > -INFINITY) {
    const float d = a.m - M, f = __expf(d);
    a.t = f * (a.t + d * a.s);
    a.s *= f;
  }
  a.m = M;
}

// column c, whose value does not exceed a.m; tv / tg: the target's value (NaN: no target) and index
__device__ __forceinline__ void add(Acc& a, float x, int c, float tv, int tg) {
  const float d = x - a.m, e = __expf(d);
  const bool fin = x > -INFINITY;  // false for NaN too
  a.s += fin ? e : 0.f;
  a.t += fin ? e * d : 0.f;  // p log p -> 0 at p = 0
  a.bad |= x != x;
  a.cnt += (x > tv || (x == tv && c < tg)) ? 1 : 0;
}

// lowest index wins a tie, whichever side it comes from
__device__ __forceinline__ void merge(Acc& a, const Acc& b) {
  const float M = fmaxf(a.m, b.m);
  if (b.m > a.m || (b.m == a.m && b.am < a.am)) a.am = b.am;  // before a.m moves
  Acc o = b;
  if (a.m < M) rescale(a, M);
  if (o.m < M) rescale(o, M);
  a.s += o.s;
  a.t += o.t;
  a.cnt += b.cnt;
  a.bad |= b.bad;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void row_stats_kernel(const float* x, int64_t ldx, const int64_t* tgt, int V, float* nll,
                                                             float* conf, float* entropy, int32_t* pred, int32_t* rank) {
  __shared__ Acc red[kWaves];
  const int row = blockIdx.x;
  const float* xr = x + (size_t)row * ldx;
  const int64_t t64 = tgt ? tgt[row] : -1;
  const bool has_t = t64 >= 0 && t64 < V;
  const int tg = has_t ? (int)t64 : -1;
  const float tv = has_t ? xr[tg] : NAN;  // NaN compares false: nothing is counted without a target
  Acc a{-INFINITY, 0.f, 0.f, 0x7fffffff, 0, 0};
  if (VEC) {
    const int n4 = V >> 2;
    for (int i = threadIdx.x; i < n4; i += kThreads) {
      const float4 v = reinterpret_cast<const float4*>(xr)[i];
      const int c = 4 * i;
      const float cm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
      if (cm > a.m) {
        rescale(a, cm);
        a.am = c + (v.x == cm ? 0 : (v.y == cm ? 1 : (v.z == cm ? 2 : 3)));
      }
      add(a, v.x, c, tv, tg);
      add(a, v.y, c + 1, tv, tg);
      add(a, v.z, c + 2, tv, tg);
      add(a, v.w, c + 3, tv, tg);
    }
    const int c = 4 * n4 + threadIdx.x;  // the V % 4 last columns
    if (c < V) {
      const float v = xr[c];
      if (v > a.m) {
        rescale(a, v);
        a.am = c;
      }
      add(a, v, c, tv, tg);
    }
  } else {
    for (int c = threadIdx.x; c < V; c += kThreads) {
      const float v = xr[c];
      if (v > a.m) {
        rescale(a, v);
        a.am = c;
      }
      add(a, v, c, tv, tg);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Acc b;
    b.m = __shfl_xor(a.m, o, 64);
    b.s = __shfl_xor(a.s, o, 64);
    b.t = __shfl_xor(a.t, o, 64);
    b.am = __shfl_xor(a.am, o, 64);
    b.cnt = __shfl_xor(a.cnt, o, 64);
    b.bad = __shfl_xor(a.bad, o, 64);
    merge(a, b);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < kWaves; ++k) merge(a, red[k]);
  const float ls = logf(a.s);
  const bool bad = a.bad != 0;
  if (nll) nll[row] = (bad || !has_t) ? NAN : (a.m - tv) + ls;  // = lse - x[target]
  if (conf) conf[row] = bad ? NAN : 1.0f / a.s;                 // = exp(max - lse)
  if (entropy) entropy[row] = bad ? NAN : ls - a.t / a.s;
  if (pred) pred[row] = bad ? -1 : a.am;
  if (rank) rank[row] = (bad || !has_t) ? -1 : a.cnt;
}

}  // namespace

extern "C" int blm_row_stats(const float* x, int64_t ldx, const int64_t* tgt, int R, int V, float* nll, float* conf, float* entropy,
                             int32_t* pred, int32_t* rank, void* stream) {
  if (!x) return blm_fail(BLM_ERR_INVALID, "blm_row_stats: null operand");
  if (R < 0 || V <= 0 || ldx < V) return blm_fail(BLM_ERR_INVALID, "blm_row_stats: bad shape");
  if (!tgt && (nll || rank)) return blm_fail(BLM_ERR_INVALID, "blm_row_stats: nll and rank need targets");
  if (!blm::extents_ok({R, (long)ldx})) return blm_fail(BLM_ERR_INVALID, "blm_row_stats: extents too large");
  if (R == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
    hipLaunchKernelGGL(row_stats_kernel<true>, dim3(R), dim3(kThreads), 0, st, x, ldx, tgt, V, nll, conf, entropy, pred, rank);
  else
    hipLaunchKernelGGL(row_stats_kernel<false>, dim3(R), dim3(kThreads), 0, st, x, ldx, tgt, V, nll, conf, entropy, pred, rank);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
