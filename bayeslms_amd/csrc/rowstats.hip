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
#include "blm_host.h"
#include "blm_rowstat.h"

namespace {

constexpr int kThreads = 256;

template <bool VEC>
__global__ __launch_bounds__(kThreads) void row_stats_kernel(const float* x, int64_t ldx, const int64_t* tgt, int V, float* nll,
                                                             float* conf, float* entropy, int32_t* pred, int32_t* rank) {
  __shared__ blm::RowAcc red[kThreads / 64];
  const int row = blockIdx.x;
  const blm::RowCols src{x + (size_t)row * ldx};
  const blm::RowTarget t = blm::row_target(tgt, row, V, src);
  blm::RowAcc a{{}, -INFINITY, 0.f, 0.f, blm::kNone, 0, 0};
  blm::row_walk<kThreads, VEC>(a, src, V, t);
  if (!blm::row_state_fold<kThreads>(a, red)) return;
  blm::row_finish(row, a, t, nll, conf, entropy, pred, rank);
}

// ---- J temperatures from one read ----
template <int J>
struct TempArgs {
  float beta[J];  // b_j
  float b2[J];    // float(b_j log2 e): exp(b_j d) = exp2(b2_j d), one multiply in front of v_exp_f32
};

// count <= J slots are written; the others ride along and leave no trace
template <int J, bool VEC>
__global__ __launch_bounds__(kThreads) void row_stats_temps_kernel(const float* x, int64_t ldx, const int64_t* tgt, int R, int V,
                                                                   TempArgs<J> tp, int count, float* nll, float* conf,
                                                                   float* entropy, float* dnll, int32_t* pred, int32_t* rank) {
#pragma clang fp contract(off)
  __shared__ blm::RowAccT<J> red[kThreads / 64];
  const int row = blockIdx.x;
  const blm::RowCols src{x + (size_t)row * ldx};
  const blm::RowTarget t = blm::row_target(tgt, row, V, src);
  blm::RowAccT<J> a;
  a.m = -INFINITY, a.am = blm::kNone, a.cnt = 0, a.bad = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) a.s[j] = a.u[j] = 0.f;
  blm::row_walk<kThreads, VEC>(a, src, V, t, tp);
  if (!blm::row_state_fold<kThreads>(a, red, tp)) return;
  const bool bad = a.bad != 0;
  const float gap = a.m - t.tv;  // max - x[target] >= 0; +inf for a target at -inf
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (j >= count) break;
    const size_t o = (size_t)j * R + row;
    const float ls = logf(a.s[j]), r = a.u[j] / a.s[j];  // r = E_b[x] - max
    blm::row_store_figures(o, bad, t.has_t, __builtin_fmaf(tp.beta[j], gap, ls), 1.0f / a.s[j], ls - tp.beta[j] * r, nll, conf,
                           entropy);
    if (dnll) dnll[o] = (bad || !t.has_t) ? NAN : gap + r;
  }
  blm::row_store_indices(row, bad, t.has_t, a.am, a.cnt, pred, rank);
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
  if (ldx % 4 == 0 && blm::aligned16(x))
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
  blm::for_slots(temps->count, [&](auto J) { launch_temps<J()>(x, ldx, tgt, R, V, temps, nll, conf, entropy, dnll, pred, rank, st); });
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
  if (ldx % 4 == 0 && blm::aligned16(x))
    hipLaunchKernelGGL(row_stats_kernel<true>, dim3(R), dim3(kThreads), 0, st, x, ldx, tgt, V, nll, conf, entropy, pred, rank);
  else
    hipLaunchKernelGGL(row_stats_kernel<false>, dim3(R), dim3(kThreads), 0, st, x, ldx, tgt, V, nll, conf, entropy, pred, rank);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
