// Word error rate of rescored n-best lists (bayeslms_amd/nbest_wer.py): word-level alignment in bulk, selection over a grid of
// score weights, and minimum-Bayes-risk selection (Stolcke, Koenig, Weintraub 1997).  include/bayeslm.h states the contract.
//
// blm_edit_distance.  A DP cell holds (cost << 16) | ins: cost and ins stay below 1024, integer `min` on the packed word is the
// lexicographic min over (cost, ins), and the rule is compositional (a step adds a constant to both fields), so the cell of the
// last row and column is the minimum cost with the fewest insertions among the minimum-cost alignments.  The sequence that
// supplies the COLUMNS plays the hypothesis (a step along a row leaves a column word unmatched: an insertion); ins - del =
// len(a) - len(b) holds for every alignment, so fewest insertions is fewest deletions and the rule does not care which of a, b
// is the columns: the kernels choose by length and exchange ins and del on the way out.  Two forms, each taking its own pairs
// of ONE launch pair (a pair is classified on the device, where the offsets live):
//   lane-per-pair   the shorter sequence is the columns, at most 32 of them, the DP row in statically indexed registers
//                   (instances for 8, 16 and 32 columns, chosen per wave by the longest of its 64 pairs); a lane walks the
//                   rows of its own pair, no lane talks to another.
//   wavefront       a wave per pair, the LONGER sequence is the columns, lane l owns columns [l C, l C + C) (C = 1, 2, 4, 8,
//                   16: 64 C >= 1023), row i is at lane l in step i + l; a step hands the lane's last cell to the next lane
//                   (one DPP wave shift) and reads the row's word from LDS.  A wave takes `ppw` consecutive pairs, ballots
//                   which of them are its form's, and works through those one after the other.
// Option "edit_lane_max" (0..32, default 32): pairs whose shorter length is at most this take the lane-per-pair form.
//
// blm_nbest_select / blm_nbest_mbr: float64, every total written out as  ac + L * (((g + w * nn) + (1 - w) * lm) + p * len)
// without contraction; reductions over (value, index) in a fixed order (lane-strided walk, xor butterfly, the four waves in
// turn through LDS) with the lowest index winning a tie: no atomics, the same bits in every run.
#include <cmath>

#include "blm_device.h"
#include "blm_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSub = 1 << 16, kDel = 1 << 16, kIns = (1 << 16) + 1;
constexpr int kRowPad = 64;  // LDS: row word i of a wave's pair is at [kRowPad + i], so that [kRowPad + step - lane] never leaves the array
constexpr int kRowWords = kRowPad + BLM_EDIT_MAX_LEN + 64 + 1;

struct Pair {
  int64_t sa, sb;  // first word of a, of b in tok
  int la, lb;      // lengths; -1: a bad pair
};

// nothing outside a / b (p < P), off[0 .. n_seq] and tok[0 .. n_tok) is read, whatever they hold
__device__ __forceinline__ Pair classify(const int64_t* off, int64_t n_tok, int n_seq, const int32_t* a, const int32_t* b, int p) {
  Pair r{0, 0, -1, -1};
  const int ia = a[p], ib = b[p];
  if ((unsigned)ia >= (unsigned)n_seq || (unsigned)ib >= (unsigned)n_seq) return r;
  const int64_t a0 = off[ia], a1 = off[ia + 1], b0 = off[ib], b1 = off[ib + 1];
  if (a0 < 0 || a1 < a0 || a1 > n_tok || a1 - a0 > BLM_EDIT_MAX_LEN) return r;
  if (b0 < 0 || b1 < b0 || b1 > n_tok || b1 - b0 > BLM_EDIT_MAX_LEN) return r;
  r.sa = a0, r.sb = b0, r.la = (int)(a1 - a0), r.lb = (int)(b1 - b0);
  return r;
}

// packed: the last cell, with the sequence of `cols_is_a` as the columns
__device__ __forceinline__ void write_out(int32_t* cost, int32_t* sid, int p, int packed, bool cols_is_a, int la, int lb) {
  const int c = packed >> 16, q = packed & 0xffff;
  cost[p] = c;
  if (sid) {
    const int ins = cols_is_a ? q : q + (la - lb), del = cols_is_a ? q - (la - lb) : q;
    sid[3 * (size_t)p] = c - ins - del;
    sid[3 * (size_t)p + 1] = ins;
    sid[3 * (size_t)p + 2] = del;
  }
}

__device__ __forceinline__ int min3(int a, int b, int c) { return min(min(a, b), c); }

// ---- lane-per-pair ----
// n <= NC columns (words at tok[sc ..]), m rows (words at tok[sr ..]); a lane without a pair of this form comes with n = m = 0
template <int NC>
__device__ __forceinline__ int lane_dp(const int32_t* tok, int64_t sc, int n, int64_t sr, int m) {
  int cw[NC], d[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    cw[j] = j < n ? tok[sc + j] : 0;
    d[j] = (j + 1) * kIns;
  }
  int d0 = 0;
  int x = m > 0 ? tok[sr] : 0;
  for (int i = 0; i < m; ++i) {
    const int xn = i + 1 < m ? tok[sr + i + 1] : 0;  // the next row's word is on its way while this row is computed
    int dg = d0;
    d0 += kDel;
    int lf = d0;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int up = d[j];
      const int v = min3(dg + (x != cw[j] ? kSub : 0), up + kDel, lf + kIns);
      d[j] = v, lf = v, dg = up;
    }
    x = xn;
  }
  int r = d0;
#pragma unroll
  for (int j = 0; j < NC; ++j) r = (n == j + 1) ? d[j] : r;
  return r;
}

__global__ __launch_bounds__(kThreads) void edit_lane_kernel(const int32_t* tok, int64_t n_tok, const int64_t* off, int n_seq,
                                                             const int32_t* a, const int32_t* b, int P, int lane_max, int32_t* cost,
                                                             int32_t* sid) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  Pair pr{0, 0, -1, -1};
  bool mine = false;
  if (p < P) {
    pr = classify(off, n_tok, n_seq, a, b, p);
    if (pr.la < 0) {
      cost[p] = -1;
      if (sid) sid[3 * (size_t)p] = sid[3 * (size_t)p + 1] = sid[3 * (size_t)p + 2] = -1;
    } else {
      mine = min(pr.la, pr.lb) <= lane_max;
    }
  }
  const bool cols_is_a = pr.la <= pr.lb;
  int n = 0, m = 0;
  if (mine) n = cols_is_a ? pr.la : pr.lb, m = cols_is_a ? pr.lb : pr.la;
  const int64_t sc = cols_is_a ? pr.sa : pr.sb, sr = cols_is_a ? pr.sb : pr.sa;
  const int rows = n > 0 ? m : 0;  // without a column the answer is m deletions: no row is walked
  int packed;
  if (__ballot(n > 16))
    packed = lane_dp<32>(tok, sc, n, sr, rows);
  else if (__ballot(n > 8))
    packed = lane_dp<16>(tok, sc, n, sr, rows);
  else
    packed = lane_dp<8>(tok, sc, n, sr, rows);
  if (n == 0) packed = m * kDel;
  if (mine) write_out(cost, sid, p, packed, cols_is_a, pr.la, pr.lb);
}

// ---- wavefront ----
// lane l takes lane l - 1's value, lane 0 keeps its own
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

// every argument but `lane` is the same in all lanes; m >= 1 columns (global words colw[0 .. m)), n <= m rows (rw[kRowPad + i])
template <int C>
__device__ __forceinline__ int wave_dp(const int32_t* colw, int m, int n, const int32_t* rw, int lane) {
  int cw[C], d[C];
  const int j0 = lane * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    cw[c] = j0 + c < m ? colw[j0 + c] : 0;
    d[c] = (j0 + c + 1) * kIns;
  }
  int diag = j0 * kIns;
  const int steps = n + (m + C - 1) / C - 1;
  int x = rw[kRowPad - lane];
  for (int t = 0; t < steps; ++t) {
    const int xn = rw[kRowPad + t + 1 - lane];
    const int recv = wave_shr1(d[C - 1]);  // lane l - 1 finished this row in the step before
    const int left = lane == 0 ? (t + 1) * kDel : recv;
    const int i = t - lane;
    if (i >= 0 && i < n) {
      int dg = diag, lf = left;
      diag = left;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int up = d[c];
        const int v = min3(dg + (x != cw[c] ? kSub : 0), up + kDel, lf + kIns);
        d[c] = v, lf = v, dg = up;
      }
    }
    x = xn;
  }
  int r = d[0];
#pragma unroll
  for (int c = 1; c < C; ++c) r = (((m - 1) & (C - 1)) == c) ? d[c] : r;
  return __shfl(r, (m - 1) / C, 64);
}

__global__ __launch_bounds__(kThreads) void edit_wave_kernel(const int32_t* tok, int64_t n_tok, const int64_t* off, int n_seq,
                                                             const int32_t* a, const int32_t* b, int P, int lane_max, int ppw,
                                                             int32_t* cost, int32_t* sid) {
  __shared__ int32_t rows[kWaves][kRowWords];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t* rw = rows[w];
  const int64_t base = ((int64_t)blockIdx.x * kWaves + w) * ppw;
  bool mine = false;
  if (lane < ppw && base + lane < P) {
    const Pair pr = classify(off, n_tok, n_seq, a, b, (int)(base + lane));
    mine = pr.la >= 0 && min(pr.la, pr.lb) > lane_max;
  }
  uint64_t todo = __ballot(mine);
  while (todo) {
    const int k = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int p = __builtin_amdgcn_readfirstlane((int)(base + k));
    const Pair pr = classify(off, n_tok, n_seq, a, b, p);  // the same in every lane
    const bool cols_is_a = pr.la >= pr.lb;
    const int m = cols_is_a ? pr.la : pr.lb, n = cols_is_a ? pr.lb : pr.la;
    const int32_t* colw = tok + (cols_is_a ? pr.sa : pr.sb);
    const int32_t* roww = tok + (cols_is_a ? pr.sb : pr.sa);
    __builtin_amdgcn_wave_barrier();  // the pair before this one has read its rows
    for (int i = lane; i < n; i += 64) rw[kRowPad + i] = roww[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int packed;
    if (m <= 64)
      packed = wave_dp<1>(colw, m, n, rw, lane);
    else if (m <= 128)
      packed = wave_dp<2>(colw, m, n, rw, lane);
    else if (m <= 256)
      packed = wave_dp<4>(colw, m, n, rw, lane);
    else if (m <= 512)
      packed = wave_dp<8>(colw, m, n, rw, lane);
    else
      packed = wave_dp<16>(colw, m, n, rw, lane);
    if (lane == 0) write_out(cost, sid, p, packed, cols_is_a, pr.la, pr.lb);
  }
}

// ---- selection ----
struct GridArgs {
  double L[BLM_NBEST_GRID_MAX], w[BLM_NBEST_GRID_MAX], p[BLM_NBEST_GRID_MAX], s[BLM_NBEST_GRID_MAX];
};

struct Costs {
  const double *ac, *g, *lm, *nn, *len;
};

struct Cost5 {
  double ac, g, lm, nn, len;
};

__device__ __forceinline__ Cost5 load5(const Costs& c, int64_t h) {
  return Cost5{c.ac ? c.ac[h] : 0.0, c.g ? c.g[h] : 0.0, c.lm ? c.lm[h] : 0.0, c.nn ? c.nn[h] : 0.0, c.len ? c.len[h] : 0.0};
}

__device__ __forceinline__ double total(const Cost5& v, double L, double w, double p) {
#pragma clang fp contract(off)
  const double a = v.g + w * v.nn;
  const double b = a + (1.0 - w) * v.lm;
  const double c = b + p * v.len;
  return v.ac + L * c;
}

__device__ __forceinline__ bool finite(double t) { return fabs(t) < INFINITY; }  // false for NaN

struct Best {
  double v;
  int i;
};

// the lower value, then the lower index
__device__ __forceinline__ void take(Best& a, const Best& b) {
  if (b.v < a.v || (b.v == a.v && b.i < a.i)) a = b;
}

// every thread gets the block's best; red: kWaves entries
__device__ __forceinline__ Best block_best(Best a, Best* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best b;
    b.v = __shfl_xor(a.v, o, 64);
    b.i = __shfl_xor(a.i, o, 64);
    take(a, b);
  }
  __syncthreads();  // red is free again
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  a = red[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) take(a, red[k]);
  return a;
}

__device__ __forceinline__ double block_sum(double a, double* red) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  a = red[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) a = a + red[k];
  return a;
}

constexpr int kNone = 0x7fffffff;

__global__ __launch_bounds__(kThreads) void nbest_select_kernel(Costs c, const int64_t* uoff, int U, GridArgs grid, int G,
                                                                int32_t* pick) {
#pragma clang fp contract(off)
  __shared__ Best red[kWaves];
  const int u = blockIdx.x;
  const int64_t lo = uoff[u], hi = uoff[u + 1];
  const int64_t N = hi > lo ? hi - lo : 0;
  const int tid = threadIdx.x;
  Cost5 first{0.0, 0.0, 0.0, 0.0, 0.0};  // a group of up to 256 is read once for the whole grid
  if (tid < N) first = load5(c, lo + tid);
  for (int gi = 0; gi < G; ++gi) {
    const double L = grid.L[gi], w = grid.w[gi], p = grid.p[gi];
    Best a{INFINITY, kNone};
    if (tid < N) {
      const double t = total(first, L, w, p);
      if (finite(t)) a = Best{t, tid};
    }
    for (int64_t i = tid + kThreads; i < N; i += kThreads) {
      const double t = total(load5(c, lo + i), L, w, p);
      if (finite(t) && t < a.v) a = Best{t, (int)i};
    }
    a = block_best(a, red);
    if (tid == 0) pick[(size_t)gi * U + u] = N == 0 ? -1 : (a.i == kNone ? 0 : a.i);
  }
}

// ---- minimum Bayes risk ----
constexpr int kChunk = 2048;  // posterior entries held in LDS at a time

__global__ __launch_bounds__(kThreads) void nbest_mbr_kernel(Costs c, const int64_t* uoff, int U, int64_t H, const int32_t* dist,
                                                             const int64_t* doff, GridArgs grid, double* risk, int32_t* pick) {
#pragma clang fp contract(off)
  __shared__ Best red[kWaves];
  __shared__ double reds[kWaves];
  __shared__ double post[kChunk];
  const int u = blockIdx.x, gi = blockIdx.y;
  const int tid = threadIdx.x;
  int64_t lo = uoff[u], hi = uoff[u + 1];
  if (lo < 0 || hi > H || hi < lo) hi = lo = 0;  // a range that leaves the arrays is an empty group
  const int64_t N = hi - lo;
  if (N == 0) {
    if (tid == 0) pick[(size_t)gi * U + u] = -1;
    return;
  }
  const double L = grid.L[gi], w = grid.w[gi], p = grid.p[gi], s = grid.s[gi];
  // the least finite total (+inf: none is finite, the posterior is then uniform)
  Best a{INFINITY, kNone};
  for (int64_t i = tid; i < N; i += kThreads) {
    const double t = total(load5(c, lo + i), L, w, p);
    if (finite(t) && t < a.v) a = Best{t, (int)i};
  }
  const double tmin = block_best(a, red).v;
  const bool uniform = !finite(tmin);
  // the unnormalised posterior of hypothesis j: the same operations wherever it is evaluated
  auto weight = [&](int64_t j) -> double {
    if (uniform) return 1.0;
    const double t = total(load5(c, lo + j), L, w, p);
    if (!finite(t)) return 0.0;
    const double e = s * (t - tmin);
    return exp(-(e / L));
  };
  double z = 0.0;
  for (int64_t j = tid; j < N; j += kThreads) z = z + weight(j);
  z = block_sum(z, reds);
  const int32_t* d = dist + doff[u];
  double* ru = risk ? risk + (size_t)gi * H + lo : nullptr;
  Best best{INFINITY, kNone};
  for (int64_t i0 = 0; i0 < N; i0 += kThreads) {
    const int64_t i = i0 + tid;
    double r = 0.0;
    for (int64_t j0 = 0; j0 < N; j0 += kChunk) {
      const int nj = (int)(N - j0 < kChunk ? N - j0 : kChunk);
      if (N > kChunk || i0 == 0) {  // a list that fits is formed once
        __syncthreads();
        for (int jj = tid; jj < nj; jj += kThreads) post[jj] = weight(j0 + jj) / z;
        __syncthreads();
      }
      if (i < N) {
        const int32_t* dj = d + j0 * N + i;  // d(j, i) = d(i, j): the block is symmetric, and this is the coalesced one
        for (int jj = 0; jj < nj; ++jj) r = r + post[jj] * (double)dj[(int64_t)jj * N];
      }
    }
    if (i < N) {
      if (ru) ru[i] = r;
      if (r < best.v) best = Best{r, (int)i};
    }
  }
  best = block_best(best, red);
  if (tid == 0) pick[(size_t)gi * U + u] = best.i == kNone ? 0 : best.i;
}

int grid_ok(const char* who, const blm_nbest_grid* grid, GridArgs* out) {
  if (grid->abi_version != BLM_ABI_VERSION)
    return blm_fail(BLM_ERR_ABI, "%s: blm_nbest_grid.abi_version %u, library %u", who, grid->abi_version, BLM_ABI_VERSION);
  if (grid->G < 1 || grid->G > BLM_NBEST_GRID_MAX)
    return blm_fail(BLM_ERR_INVALID, "%s: G %d outside 1..%d", who, grid->G, BLM_NBEST_GRID_MAX);
  for (int i = 0; i < BLM_NBEST_GRID_MAX; ++i) {
    const int k = i < grid->G ? i : 0;  // the surplus slots repeat point 0 and are never read
    if (!(grid->lmwt[k] > 0.0) || !std::isfinite(grid->lmwt[k]))
      return blm_fail(BLM_ERR_INVALID, "%s: lmwt[%d] = %g is not a positive finite LM weight", who, k, grid->lmwt[k]);
    if (!(grid->pscale[k] >= 0.0) || !std::isfinite(grid->pscale[k]))
      return blm_fail(BLM_ERR_INVALID, "%s: pscale[%d] = %g is not a finite posterior scale >= 0", who, k, grid->pscale[k]);
    out->L[i] = grid->lmwt[k], out->w[i] = grid->nnweight[k], out->p[i] = grid->wip[k], out->s[i] = grid->pscale[k];
  }
  return BLM_OK;
}

}  // namespace

extern "C" int blm_edit_distance(const int32_t* tok, int64_t n_tok, const int64_t* off, int n_seq, const int32_t* a, const int32_t* b,
                                 int P, int32_t* cost, int32_t* sid, void* stream) {
  if (!off || !a || !b || !cost) return blm_fail(BLM_ERR_INVALID, "blm_edit_distance: null operand");
  if (n_tok < 0 || n_seq < 0 || P < 0) return blm_fail(BLM_ERR_INVALID, "blm_edit_distance: negative count");
  if (!tok && n_tok > 0) return blm_fail(BLM_ERR_INVALID, "blm_edit_distance: null tok");
  if (n_tok > blm::kMaxExtent || !blm::extents_ok({(long)n_seq + 1}) || !blm::extents_ok({P, 3}))
    return blm_fail(BLM_ERR_INVALID, "blm_edit_distance: extents too large");
  if (P == 0) return BLM_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int lane_max = blm::option(blm::OPT_EDIT_LANE_MAX);
  hipLaunchKernelGGL(edit_lane_kernel, dim3((P + kThreads - 1) / kThreads), dim3(kThreads), 0, st, tok, n_tok, off, n_seq, a, b, P,
                     lane_max, cost, sid);
  BLM_HIP(hipGetLastError());
  // pairs a wave works through: one while that still gives every SIMD several waves, up to 64 for long lists
  const int ppw = P / 8192 < 1 ? 1 : (P / 8192 > 64 ? 64 : P / 8192);
  const int waves = (P + ppw - 1) / ppw;
  hipLaunchKernelGGL(edit_wave_kernel, dim3((waves + kWaves - 1) / kWaves), dim3(kThreads), 0, st, tok, n_tok, off, n_seq, a, b, P,
                     lane_max, ppw, cost, sid);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_nbest_select(const double* ac, const double* g, const double* lm, const double* nn, const double* len,
                                const int64_t* uoff, int U, const blm_nbest_grid* grid, int32_t* pick, void* stream) {
  if (!uoff || !grid || !pick) return blm_fail(BLM_ERR_INVALID, "blm_nbest_select: null operand");
  if (U < 0) return blm_fail(BLM_ERR_INVALID, "blm_nbest_select: negative count");
  GridArgs ga;
  if (const int rc = grid_ok("blm_nbest_select", grid, &ga)) return rc;
  if (!blm::extents_ok({(long)U + 1}) || !blm::extents_ok({U, BLM_NBEST_GRID_MAX}))
    return blm_fail(BLM_ERR_INVALID, "blm_nbest_select: extents too large");
  if (U == 0) return BLM_OK;
  hipLaunchKernelGGL(nbest_select_kernel, dim3(U), dim3(kThreads), 0, static_cast<hipStream_t>(stream), Costs{ac, g, lm, nn, len},
                     uoff, U, ga, (int)grid->G, pick);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_nbest_mbr(const double* ac, const double* g, const double* lm, const double* nn, const double* len,
                             const int64_t* uoff, int U, int64_t H, const int32_t* dist, const int64_t* doff,
                             const blm_nbest_grid* grid, double* risk, int32_t* pick, void* stream) {
  if (!uoff || !dist || !doff || !grid || !pick) return blm_fail(BLM_ERR_INVALID, "blm_nbest_mbr: null operand");
  if (U < 0 || H < 0) return blm_fail(BLM_ERR_INVALID, "blm_nbest_mbr: negative count");
  GridArgs ga;
  if (const int rc = grid_ok("blm_nbest_mbr", grid, &ga)) return rc;
  if (H > blm::kMaxExtent || !blm::extents_ok({(long)U + 1}) || !blm::extents_ok({U, BLM_NBEST_GRID_MAX}) ||
      !blm::extents_ok({(long)H, BLM_NBEST_GRID_MAX}))
    return blm_fail(BLM_ERR_INVALID, "blm_nbest_mbr: extents too large");
  if (U == 0) return BLM_OK;
  hipLaunchKernelGGL(nbest_mbr_kernel, dim3(U, grid->G), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     Costs{ac, g, lm, nn, len}, uoff, U, H, dist, doff, ga, risk, pick);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
