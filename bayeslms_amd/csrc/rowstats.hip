// Row statistics of a matrix of logits or log-probabilities (engine.evaluate_report): per row the target's NLL, the
// confidence (largest probability), the entropy, the prediction and the target's rank, from ONE read of the row.  Vector ALU,
// bound by the bytes it reads: one 256-thread workgroup per row, every lane carries an online softmax state (running max and its
// lowest index, sum of exp(x - max), sum of exp(x - max) (x - max), rank count) that is rescaled when its max moves, and the
// lanes' states are merged in a fixed order (xor butterfly inside a wave, then the four waves in turn through LDS): no atomics,
// the same bits in every run.
//
// blm_row_stats_temps (engine.evaluate_temperatures / fit_temperature) is the same walk for J <= BLM_ROW_TEMPS_MAX inverse
// temperatures at once: the tempered distribution p_b ~ exp(b x) of every b in the list from the SAME single read of the row.
// The running max with its lowest index, the rank count and the NaN flag do not depend on b > 0 and are carried once; per
// temperature a lane carries s_j = sum exp(b_j d) and u_j = sum exp(b_j d) d with d = x - max UNSCALED, so that
// nll = b (max - x_t) + log s, entropy = log s - b u / s and d nll / d b = (max - x_t) + u / s.  The list travels in the kernel
// arguments (no device allocation, no copy).  Slot j runs the same operations in the same order whatever J is and whatever the
// other slots hold (fused multiply-adds are written out and contraction is off in these functions, so the compiler has no
// choice to make differently from one form to the next): its figures are bit-identical alone, in a longer list and at another
// position.
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

// ---- J temperatures from one read ----
template <int J>
struct TempArgs {
  float beta[J];  // b_j
  float b2[J];    // float(b_j log2 e): exp(b_j d) = exp2(b2_j d), one multiply in front of v_exp_f32
};

template <int J>
struct TAcc {
  float m;
  int am, cnt, bad;
  float s[J], u[J];
};

// the state re-expressed for a max M > a.m (a.m == -inf: nothing summed yet, s = u = 0 stay)
template <int J>
__device__ __forceinline__ void trescale(TAcc<J>& a, float M, const TempArgs<J>& tp) {
#pragma clang fp contract(off)
  if (a.m > -INFINITY) {
    const float d = a.m - M;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float f = __builtin_amdgcn_exp2f(tp.b2[j] * d);
      a.u[j] = f * __builtin_fmaf(d, a.s[j], a.u[j]);
      a.s[j] = f * a.s[j];
    }
  }
  a.m = M;
}

template <int J>
__device__ __forceinline__ void tadd(TAcc<J>& a, float x, int c, float tv, int tg, const TempArgs<J>& tp) {
#pragma clang fp contract(off)
  const bool fin = x > -INFINITY;  // false for NaN too
  const float dx = x - a.m;
  const float de = fin ? dx : -INFINITY;  // b2 > 0: exp2(b2 * -inf) = 0, one select for all J instead of one each
  const float d = fin ? dx : 0.f;         // p log p -> 0 at p = 0
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const float e = __builtin_amdgcn_exp2f(tp.b2[j] * de);
    a.s[j] += e;
    a.u[j] = __builtin_fmaf(e, d, a.u[j]);
  }
  a.bad |= x != x;
  a.cnt += (x > tv || (x == tv && c < tg)) ? 1 : 0;
}

template <int J>
__device__ __forceinline__ void tmerge(TAcc<J>& a, const TAcc<J>& b, const TempArgs<J>& tp) {
#pragma clang fp contract(off)
  const float M = fmaxf(a.m, b.m);
  if (b.m > a.m || (b.m == a.m && b.am < a.am)) a.am = b.am;  // before a.m moves
  TAcc<J> o = b;
  if (a.m < M) trescale(a, M, tp);
  if (o.m < M) trescale(o, M, tp);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    a.s[j] += o.s[j];
    a.u[j] += o.u[j];
  }
  a.cnt += b.cnt;
  a.bad |= b.bad;
}

// count <= J slots are written; the others ride along and leave no trace
template <int J, bool VEC>
__global__ __launch_bounds__(kThreads) void row_stats_temps_kernel(const float* x, int64_t ldx, const int64_t* tgt, int R, int V,
                                                                   TempArgs<J> tp, int count, float* nll, float* conf,
                                                                   float* entropy, float* dnll, int32_t* pred, int32_t* rank) {
#pragma clang fp contract(off)
  __shared__ TAcc<J> red[kWaves];
  const int row = blockIdx.x;
  const float* xr = x + (size_t)row * ldx;
  const int64_t t64 = tgt ? tgt[row] : -1;
  const bool has_t = t64 >= 0 && t64 < V;
  const int tg = has_t ? (int)t64 : -1;
  const float tv = has_t ? xr[tg] : NAN;  // NaN compares false: nothing is counted without a target
  TAcc<J> a;
  a.m = -INFINITY, a.am = 0x7fffffff, a.cnt = 0, a.bad = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) a.s[j] = a.u[j] = 0.f;
  if (VEC) {
    const int n4 = V >> 2;
    for (int i = threadIdx.x; i < n4; i += kThreads) {
      const float4 v = reinterpret_cast<const float4*>(xr)[i];
      const int c = 4 * i;
      const float cm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
      if (cm > a.m) {
        trescale(a, cm, tp);
        a.am = c + (v.x == cm ? 0 : (v.y == cm ? 1 : (v.z == cm ? 2 : 3)));
      }
      tadd(a, v.x, c, tv, tg, tp);
      tadd(a, v.y, c + 1, tv, tg, tp);
      tadd(a, v.z, c + 2, tv, tg, tp);
      tadd(a, v.w, c + 3, tv, tg, tp);
    }
    const int c = 4 * n4 + threadIdx.x;  // the V % 4 last columns
    if (c < V) {
      const float v = xr[c];
      if (v > a.m) {
        trescale(a, v, tp);
        a.am = c;
      }
      tadd(a, v, c, tv, tg, tp);
    }
  } else {
    for (int c = threadIdx.x; c < V; c += kThreads) {
      const float v = xr[c];
      if (v > a.m) {
        trescale(a, v, tp);
        a.am = c;
      }
      tadd(a, v, c, tv, tg, tp);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    TAcc<J> b;
    b.m = __shfl_xor(a.m, o, 64);
    b.am = __shfl_xor(a.am, o, 64);
    b.cnt = __shfl_xor(a.cnt, o, 64);
    b.bad = __shfl_xor(a.bad, o, 64);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      b.s[j] = __shfl_xor(a.s[j], o, 64);
      b.u[j] = __shfl_xor(a.u[j], o, 64);
    }
    tmerge(a, b, tp);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < kWaves; ++k) tmerge(a, red[k], tp);
  const bool bad = a.bad != 0;
  const float gap = a.m - tv;  // max - x[target] >= 0; +inf for a target at -inf
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (j >= count) break;
    const size_t o = (size_t)j * R + row;
    const float ls = logf(a.s[j]), r = a.u[j] / a.s[j];  // r = E_b[x] - max
    if (nll) nll[o] = (bad || !has_t) ? NAN : __builtin_fmaf(tp.beta[j], gap, ls);
    if (conf) conf[o] = bad ? NAN : 1.0f / a.s[j];
    if (entropy) entropy[o] = bad ? NAN : ls - tp.beta[j] * r;
    if (dnll) dnll[o] = (bad || !has_t) ? NAN : gap + r;
  }
  if (pred) pred[row] = bad ? -1 : a.am;
  if (rank) rank[row] = (bad || !has_t) ? -1 : a.cnt;
}

template <int J>
void launch_temps(const float* x, int64_t ldx, const int64_t* tgt, int R, int V, const blm_row_temps* t, float* nll, float* conf,
                  float* entropy, float* dnll, int32_t* pred, int32_t* rank, hipStream_t st) {
  TempArgs<J> tp;
  for (int j = 0; j < J; ++j) {
    const float b = t->beta[j < t->count ? j : 0];  // a surplus slot repeats slot 0: any b > 0 keeps its sums finite
    tp.beta[j] = b;
    tp.b2[j] = (float)((double)b * 1.4426950408889634);
  }
  if (ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
    hipLaunchKernelGGL((row_stats_temps_kernel<J, true>), dim3(R), dim3(kThreads), 0, st, x, ldx, tgt, R, V, tp, (int)t->count, nll,
                       conf, entropy, dnll, pred, rank);
  else
    hipLaunchKernelGGL((row_stats_temps_kernel<J, false>), dim3(R), dim3(kThreads), 0, st, x, ldx, tgt, R, V, tp, (int)t->count, nll,
                       conf, entropy, dnll, pred, rank);
}

}  // namespace

extern "C" int blm_row_stats_temps(const float* x, int64_t ldx, const int64_t* tgt, int R, int V, const blm_row_temps* temps,
                                   float* nll, float* conf, float* entropy, float* dnll, int32_t* pred, int32_t* rank,
                                   void* stream) {
  if (!x || !temps) return blm_fail(BLM_ERR_INVALID, "blm_row_stats_temps: null operand");
  if (temps->abi_version != BLM_ABI_VERSION)
    return blm_fail(BLM_ERR_ABI, "blm_row_stats_temps: blm_row_temps.abi_version %u, library %u", temps->abi_version, BLM_ABI_VERSION);
  if (temps->count < 1 || temps->count > BLM_ROW_TEMPS_MAX)
    return blm_fail(BLM_ERR_INVALID, "blm_row_stats_temps: count %d outside 1..%d", temps->count, BLM_ROW_TEMPS_MAX);
  for (int j = 0; j < temps->count; ++j)
    if (!(temps->beta[j] > 0.f) || !(temps->beta[j] <= 3.402823466e38f))
      return blm_fail(BLM_ERR_INVALID, "blm_row_stats_temps: beta[%d] = %g is not a positive finite inverse temperature", j,
                      (double)temps->beta[j]);
  if (R < 0 || V <= 0 || ldx < V) return blm_fail(BLM_ERR_INVALID, "blm_row_stats_temps: bad shape");
  if (!tgt && (nll || dnll || rank)) return blm_fail(BLM_ERR_INVALID, "blm_row_stats_temps: nll, dnll and rank need targets");
  if (!blm::extents_ok({R, (long)ldx}) || !blm::extents_ok({R, (long)BLM_ROW_TEMPS_MAX}))
    return blm_fail(BLM_ERR_INVALID, "blm_row_stats_temps: extents too large");
  if (R == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int J = temps->count;
  if (J == 1)
    launch_temps<1>(x, ldx, tgt, R, V, temps, nll, conf, entropy, dnll, pred, rank, st);
  else if (J == 2)
    launch_temps<2>(x, ldx, tgt, R, V, temps, nll, conf, entropy, dnll, pred, rank, st);
  else if (J <= 4)
    launch_temps<4>(x, ldx, tgt, R, V, temps, nll, conf, entropy, dnll, pred, rank, st);
  else
    launch_temps<8>(x, ldx, tgt, R, V, temps, nll, conf, entropy, dnll, pred, rank, st);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

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
