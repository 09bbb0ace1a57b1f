// Search on the incremental path (bayeslms_amd/incremental.py beam_search, generate.py): the k best entries of every row
// (blm_topk_rows), the B best continuations of every group of B beams (blm_beam_select), the same step with a pool of finished
// hypotheses beside the beam (blm_beam_select_pool) and Gumbel-max sampling restricted to a top-k / nucleus prefix of the row's
// order (blm_sample_rows_filtered).
//
// One device routine serves all four: a most-significant-digit radix select over 64-bit composites
//     c(i) = order_key(value i) << nb  |  (2^nb - 1 - i)              nb = bits of the largest index
// order_key maps a float to 32 bits so that a larger key is a better entry (value descending, -0 == +0, every NaN below -inf),
// and the inverted index below it makes "lowest index first among equal values" part of the same integer order.  Composites
// are distinct, so "the n best entries" is exactly { i : c(i) >= C* } for one threshold C*, which the select finds in at most
// ceil((32 + nb) / 8) passes of a 256-bin histogram in LDS (integer atomics only: the result does not depend on the order in
// which waves arrive, and nothing is recomputed in floating point).  A pass ends the select early when the whole threshold
// bin is taken.  The row is re-read from L2 in every pass (a 33,000-float row is 132 KB; the LDS-resident form was not built).
#include "blm_device.h"
#include "blm_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTopkMax = BLM_TOPK_MAX;
static_assert(kTopkMax == kThreads, "the bitonic sort below holds one survivor per thread");
typedef unsigned long long u64;

// larger key = better entry; 0 is kept for "no such candidate", 1 for NaN
__device__ __forceinline__ uint32_t order_key(float x) {
  if (x != x) return 1u;
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;  // -0 == +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct SelSmem {
  u64 hist_c[256];  // entries per bin
  u64 hist_m[256];  // fixed-point probability mass per bin (mass mode)
  u64 wsum[kThreads / 64];
  u64 pick[4];      // bin, entries of the bin, what is still wanted inside the bin, entries of the bins above
  u64 surv[kTopkMax];
  int nsurv;
};

__device__ __forceinline__ int index_bits(int n) {
  int nb = 1;
  while (nb < 30 && (1 << nb) < n) ++nb;
  return nb;
}

// inclusive prefix sum over the thread index; safe to call again right after it returns
__device__ __forceinline__ u64 block_scan(u64 v, u64* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) wsum[w] = v;
  __syncthreads();
  for (int i = 0; i < w; ++i) v += wsum[i];
  __syncthreads();
  return v;
}

// hist[bin] += 1 for the active lanes.  The top digits of a row of log-probabilities fall into a handful of bins, and a
// wave's 64 atomics on one LDS word run one after the other: the four most common bins of the wave are counted by ballot.
__device__ __forceinline__ void hist_count(u64* hist, bool act, int bin) {
  const int lane = threadIdx.x & 63;
  for (int it = 0; it < 4; ++it) {
    const u64 rem = __ballot(act);
    if (!rem) return;
    const int leader = __ffsll((long long)rem) - 1;
    const int lb = __shfl(bin, leader, 64);
    const bool mine = act && bin == lb;
    const u64 same = __ballot(mine);
    if (lane == leader) atomicAdd(&hist[lb], (u64)__popcll(same));
    if (mine) act = false;
  }
  if (act) atomicAdd(&hist[bin], 1ull);
}

// The threshold composite C* of the `want` best of n entries (MASS false: want is a count, 1 <= want <= n) or of the
// shortest prefix of the order whose mass reaches `want` (MASS true: 1 <= want <= total mass).  key(i) -> order key of entry
// i, mass(i) -> its fixed-point mass.  Returns C*; *taken = entries with c >= C*.  Every thread of the block must call it.
template <bool MASS, class KeyFn, class MassFn>
__device__ u64 radix_select(KeyFn key, MassFn mass, int n, u64 want, SelSmem& sm, u64* taken) {
  const int nb = index_bits(n);
  const uint32_t imask = (1u << nb) - 1u;
  const int npass = (32 + nb + 7) / 8;
  u64 prefix = 0, above = 0;
  for (int p = 0; p < npass; ++p) {
    const int shift = 8 * (npass - 1 - p);
    sm.hist_c[threadIdx.x] = 0;
    if (MASS) sm.hist_m[threadIdx.x] = 0;
    __syncthreads();
    for (int base = 0; base < n; base += kThreads) {  // whole waves stay in the loop: hist_count uses ballots
      const int i = base + threadIdx.x;
      bool act = i < n;
      u64 c = 0;
      if (act) {
        c = ((u64)key(i) << nb) | (u64)(imask - (uint32_t)i);
        act = p == 0 || (c >> (shift + 8)) == prefix;
      }
      const int bin = (int)((c >> shift) & 255);
      if (MASS) {
        if (act) {
          atomicAdd(&sm.hist_c[bin], 1ull);
          atomicAdd(&sm.hist_m[bin], mass(i));
        }
      } else {
        hist_count(sm.hist_c, act, bin);
      }
    }
    __syncthreads();
    // thread t owns bin 255 - t: the scan runs from the best bin down
    const int b = 255 - threadIdx.x;
    const u64 cnt = sm.hist_c[b];
    const u64 inc_c = block_scan(cnt, sm.wsum);
    u64 amt = cnt, inc = inc_c;
    if (MASS) {
      amt = sm.hist_m[b];
      inc = block_scan(amt, sm.wsum);
    }
    if (threadIdx.x == 0) sm.pick[1] = 0;
    __syncthreads();
    if (amt > 0 && inc >= want && inc - amt < want) {
      sm.pick[0] = (u64)b;
      sm.pick[1] = cnt;
      sm.pick[2] = want - (inc - amt);
      sm.pick[3] = inc_c - cnt;
    }
    __syncthreads();
    const u64 bin = sm.pick[0], bcnt = sm.pick[1];
    if (bcnt == 0) {  // fewer entries (or less mass) than wanted: everything qualifies
      *taken = (u64)n;
      return 0;
    }
    want = sm.pick[2];
    above += sm.pick[3];
    prefix = (prefix << 8) | bin;
    __syncthreads();  // pick[] is read before the next pass overwrites it
    if (MASS ? bcnt == 1 : want == bcnt) {  // the whole bin is taken: no lower digit can split it
      *taken = above + bcnt;
      return prefix << shift;
    }
  }
  *taken = above + 1;  // not reached: composites are distinct, so the last pass ends with a bin of one entry
  return prefix;
}

struct NoMass {
  __device__ u64 operator()(int) const { return 0; }
};

// Every entry with c >= cstar goes into sm.surv (at most kTopkMax of them), which is then sorted best first.  `n_out` slots
// are valid afterwards; slots past the survivors hold 0.
template <class KeyFn>
__device__ void collect_sorted(KeyFn key, int n, u64 cstar, int n_out, SelSmem& sm) {
  const int nb = index_bits(n);
  const uint32_t imask = (1u << nb) - 1u;
  sm.surv[threadIdx.x] = 0;
  if (threadIdx.x == 0) sm.nsurv = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const u64 c = ((u64)key(i) << nb) | (u64)(imask - (uint32_t)i);
    if (c >= cstar) {
      const int pos = atomicAdd(&sm.nsurv, 1);  // any slot: the sort below fixes the order
      if (pos < kTopkMax) sm.surv[pos] = c;
    }
  }
  __syncthreads();
  int len = 1;
  while (len < n_out) len <<= 1;
  for (int k = 2; k <= len; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int t = threadIdx.x, o = t ^ j;
      if (t < len && o > t) {
        const u64 a = sm.surv[t], b = sm.surv[o];
        const bool desc = (t & k) == 0;
        if (desc ? a < b : a > b) {
          sm.surv[t] = b;
          sm.surv[o] = a;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kThreads) void topk_rows_kernel(const float* x, int64_t ldx, int V, int k, float* vals, int64_t* ids) {
  __shared__ SelSmem sm;
  const float* xr = x + (size_t)blockIdx.x * ldx;
  auto key = [xr](int i) { return order_key(xr[i]); };
  u64 taken;
  const u64 cstar = radix_select<false>(key, NoMass(), V, (u64)k, sm, &taken);
  collect_sorted(key, V, cstar, k, sm);
  const uint32_t imask = (1u << index_bits(V)) - 1u;
  if (threadIdx.x < k) {
    const int i = (int)(imask - (uint32_t)(sm.surv[threadIdx.x] & imask));
    if (i < V) {
      vals[(size_t)blockIdx.x * k + threadIdx.x] = xr[i];
      ids[(size_t)blockIdx.x * k + threadIdx.x] = i;
    }
  }
}

__global__ __launch_bounds__(kThreads) void beam_select_kernel(const float* cand_vals, const int64_t* cand_ids, const float* score,
                                                               const uint8_t* finished, int B, int k, int64_t eos, float* score_out,
                                                               uint8_t* finished_out, int64_t* parent, int64_t* token) {
  __shared__ SelSmem sm;
  const int g0 = blockIdx.x * B, n = B * k;
  // flat candidate b * k + j; a finished beam has the one candidate j = 0 (itself)
  auto cand = [=](int i) {
    const int b = i / k;
    return finished[g0 + b] ? score[g0 + b] : score[g0 + b] + cand_vals[(size_t)g0 * k + i];
  };
  auto key = [=](int i) {
    const int b = i / k;
    if (finished[g0 + b] && i != b * k) return 0u;
    return order_key(cand(i));
  };
  u64 taken;
  const u64 cstar = radix_select<false>(key, NoMass(), n, (u64)B, sm, &taken);
  collect_sorted(key, n, cstar, B, sm);
  const uint32_t imask = (1u << index_bits(n)) - 1u;
  if (threadIdx.x < B) {
    const int i = (int)(imask - (uint32_t)(sm.surv[threadIdx.x] & imask));
    if (i < n) {
      const int b = i / k;
      const bool fin = finished[g0 + b] != 0;
      const int64_t tok = fin ? eos : cand_ids[(size_t)g0 * k + i];
      score_out[g0 + threadIdx.x] = cand(i);
      finished_out[g0 + threadIdx.x] = (fin || tok == eos) ? 1 : 0;
      parent[g0 + threadIdx.x] = g0 + b;
      token[g0 + threadIdx.x] = tok;
    }
  }
}

struct PoolSmem {
  uint32_t okey[kTopkMax];  // order keys of the norms the pool holds before the step, in pool order
  uint32_t nkey[kTopkMax];  // of the entries offered at this step, in insertion order (at most B eos + B flushed <= kTopkMax)
  int n_cont, n_eos;        // candidates of the walk that are not eos / eos of rank < B
  float best;               // score of new beam 0
  uint32_t last_key;        // key of the full pool's last norm after the step
};

// blm_beam_select_pool (include/bayeslm.h).  The walk needs the first 2 B ranks only: one select + sort of them, a scan that
// numbers the eos and the other candidates, and a merge of the offered entries into the pool by counting, for every entry, the
// entries that precede it -- the pool is sorted and the offered ones are numbered, so ranks are distinct and every write has
// its own slot.  All of the old pool is in registers before the first write to it.
__global__ __launch_bounds__(kThreads) void beam_select_pool_kernel(const float* cand_vals, const int64_t* cand_ids, const float* score,
                                                                    const uint8_t* live, int B, int k, int64_t eos, int step, int len,
                                                                    int min_len, float inv_norm, float inv_norm_max, int flush,
                                                                    blm_beam_pool pool, float* score_out, uint8_t* live_out,
                                                                    int64_t* parent, int64_t* token, uint8_t* done_out) {
  __shared__ SelSmem sm;
  __shared__ PoolSmem ps;
  const int t = threadIdx.x, g = blockIdx.x, g0 = g * B, n = B * k, P = pool.P;
  const int want = min(2 * B, n);
  const float* cv = cand_vals + (size_t)g0 * k;
  const int64_t* ci = cand_ids + (size_t)g0 * k;
  auto cand = [=](int i) { return score[g0 + i / k] + cv[i]; };
  auto key = [=](int i) {
    if (!live[g0 + i / k]) return 0u;
    const float s = cand(i);
    if (!(s > -INFINITY)) return 0u;  // NaN or -inf
    if (len < min_len && ci[i] == eos) return 0u;
    return order_key(s);
  };
  u64 taken;
  const u64 cstar = radix_select<false>(key, NoMass(), n, (u64)want, sm, &taken);
  collect_sorted(key, n, cstar, want, sm);
  const int nb = index_bits(n);
  const uint32_t imask = (1u << nb) - 1u;
  // thread t holds rank t of the walk
  bool is_eos = false, cont = false;
  int b = 0;
  float s = 0.f;
  int64_t tok = eos;
  if (t < want) {
    const u64 c = sm.surv[t];
    const int i = (int)(imask - (uint32_t)(c & imask));
    if ((c >> nb) != 0 && i < n) {
      b = i / k;
      s = cand(i);
      tok = ci[i];
      is_eos = tok == eos;
      cont = !is_eos;
    }
  }
  const bool pooled = is_eos && t < B;
  const u64 inc = block_scan((u64)(cont ? 1 : 0) | ((u64)(pooled ? 1 : 0) << 32), sm.wsum);
  const int slot = (int)(uint32_t)inc - (cont ? 1 : 0);  // candidates that are not eos before this one
  if (t == kThreads - 1) {
    ps.n_cont = (int)(uint32_t)inc;
    ps.n_eos = (int)(inc >> 32);
    ps.best = -INFINITY;
    ps.last_key = 0;
  }
  __syncthreads();
  const int n_live = min(ps.n_cont, B), n_eos = ps.n_eos;
  const bool beam = cont && slot < B;
  const int n_new = n_eos + (flush ? n_live : 0);
  // the entry this thread offers (at most one), numbered in insertion order
  const bool offers = pooled || (beam && flush);
  const int q = pooled ? (int)(inc >> 32) - 1 : n_eos + slot;
  const float norm = __fmul_rn(s, inv_norm);
  if (offers) ps.nkey[q] = order_key(norm);
  if (beam && slot == 0) ps.best = s;
  // the entry of the pool this thread moves
  const size_t p0 = (size_t)g * P;
  const int count = min(max(pool.count[g], 0), P);
  float o_norm = 0.f, o_raw = 0.f;
  int o_len = 0, o_step = 0;
  int64_t o_parent = 0;
  uint8_t o_fin = 0;
  if (t < count) {
    o_norm = pool.norm[p0 + t];
    o_raw = pool.raw[p0 + t];
    o_len = pool.len[p0 + t];
    o_step = pool.step[p0 + t];
    o_parent = pool.parent[p0 + t];
    o_fin = pool.finished[p0 + t];
    ps.okey[t] = order_key(o_norm);
  }
  __syncthreads();
  const int n_after = min(P, count + n_new);
  if (n_new > 0 && t < count) {
    const uint32_t mine = ps.okey[t];
    int r = t;
    for (int j = 0; j < n_new; ++j) r += ps.nkey[j] > mine ? 1 : 0;
    if (r < P && r != t) {
      pool.norm[p0 + r] = o_norm;
      pool.raw[p0 + r] = o_raw;
      pool.len[p0 + r] = o_len;
      pool.step[p0 + r] = o_step;
      pool.parent[p0 + r] = o_parent;
      pool.finished[p0 + r] = o_fin;
    }
    if (r == P - 1) ps.last_key = mine;
  } else if (t == P - 1 && t < count) {
    ps.last_key = ps.okey[t];
  }
  if (offers) {
    const uint32_t mine = ps.nkey[q];
    int r = 0;
    for (int j = 0; j < count; ++j) r += ps.okey[j] >= mine ? 1 : 0;
    for (int j = 0; j < n_new; ++j) r += (ps.nkey[j] > mine || (ps.nkey[j] == mine && j < q)) ? 1 : 0;
    if (r < P) {
      pool.norm[p0 + r] = norm;
      pool.raw[p0 + r] = s;
      pool.len[p0 + r] = len;
      pool.step[p0 + r] = step;
      pool.parent[p0 + r] = pooled ? g0 + b : g0 + slot;
      pool.finished[p0 + r] = pooled ? 1 : 0;
    }
    if (r == P - 1) ps.last_key = mine;
  }
  __syncthreads();
  const bool done = n_live == 0 || flush || (n_after == P && order_key(__fmul_rn(ps.best, inv_norm_max)) < ps.last_key);
  if (beam) {
    score_out[g0 + slot] = done ? -INFINITY : s;
    live_out[g0 + slot] = done ? 0 : 1;
    parent[g0 + slot] = g0 + b;
    token[g0 + slot] = tok;
  }
  if (t >= n_live && t < B) {
    score_out[g0 + t] = -INFINITY;
    live_out[g0 + t] = 0;
    parent[g0 + t] = g0 + t;
    token[g0 + t] = eos;
  }
  if (t == 0) {
    pool.count[g] = n_after;
    pool.inserted[g] += n_new;
    done_out[g] = done ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads) void all_done_kernel(const uint8_t* done, int G, uint8_t* all_done) {
  int ok = 1;
  for (int i = threadIdx.x; i < G; i += kThreads) ok &= done[i] != 0;
  ok = __syncthreads_and(ok);
  if (threadIdx.x == 0) *all_done = ok ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void sample_rows_filtered_kernel(const float* x, int64_t ldx, int V, float inv_t, int greedy,
                                                                        int top_k, float top_p, blm_rng rng, int64_t* out) {
  __shared__ SelSmem sm;
  __shared__ float red[kThreads / 64];
  __shared__ float sv[kThreads / 64];
  __shared__ int si[kThreads / 64];
  const int row = blockIdx.x;
  const float* xr = x + (size_t)row * ldx;
  auto key = [xr](int i) { return order_key(xr[i]); };
  u64 cstar = 0;  // every entry is allowed
  if (!greedy) {
    int n_allowed = top_k > 0 && top_k < V ? top_k : V;
    if (top_p < 1.f) {
      // q = softmax(x / temperature) as integers: e = exp(x / t - max) in (0, 1] times 2^sh, sh chosen so that V of them fit
      // 62 bits.  Integer sums do not depend on their order, so the mass of a bin and the cut are the same in every run.
      float m = -INFINITY;
      for (int c = threadIdx.x; c < V; c += kThreads) m = fmaxf(m, xr[c] * inv_t);
      m = blm::block_max<kThreads / 64>(m, red);
      const int sh = min(40, 62 - index_bits(V));
      const float scale = __uint_as_float((uint32_t)(127 + sh) << 23);
      auto mass = [=](int i) -> u64 {
        const float z = xr[i] * inv_t;
        const float e = z == m ? 1.f : expf(z - m);
        return e == e ? (u64)(e * scale) : 0ull;
      };
      u64 part = 0;
      for (int c = threadIdx.x; c < V; c += kThreads) part += mass(c);
      const u64 inc = block_scan(part, sm.wsum);
      if (threadIdx.x == kThreads - 1) sm.pick[0] = inc;
      __syncthreads();
      const u64 total = sm.pick[0];
      __syncthreads();
      if (total > 0) {
        const double t = ceil((double)top_p * (double)total);
        u64 want = t >= (double)total ? total : (u64)t;
        if (want < 1) want = 1;
        u64 n_p;
        cstar = radix_select<true>(key, mass, V, want, sm, &n_p);
        if (n_p <= (u64)n_allowed)
          n_allowed = (int)n_p;  // the nucleus is the shorter prefix: its threshold stands
        else
          cstar = 0;
      }
    }
    if (cstar == 0 && n_allowed < V) {
      u64 taken;
      cstar = radix_select<false>(key, NoMass(), V, (u64)n_allowed, sm, &taken);
    }
  }
  const int nb = index_bits(V);
  const uint32_t imask = (1u << nb) - 1u;
  blm::Best b = {-INFINITY, blm::kNone};
  for (int c = threadIdx.x; c < V; c += kThreads) {
    float s = xr[c];
    if (cstar != 0 && (((u64)order_key(s) << nb) | (u64)(imask - (uint32_t)c)) < cstar) continue;
    if (!greedy) {
      const blm::u32x4 u = blm::philox4x32_10((uint32_t)c, (uint32_t)row, rng.stream, rng.step, (uint32_t)rng.seed,
                                              (uint32_t)(rng.seed >> 32));
      const float uu = ((float)(u.x >> 8) + 0.5f) * 5.9604644775390625e-08f;  // (0, 1)
      s = s * inv_t - logf(-logf(uu));                                         // Gumbel-max
    }
    blm::best_of(b, s, c);
  }
  blm::block_best<kThreads / 64>(b, sv, si);
  if (threadIdx.x == 0) out[row] = b.i == blm::kNone ? 0 : b.i;
}

}  // namespace

extern "C" int blm_topk_rows(const float* x, int64_t ldx, int R, int V, int k, float* vals, int64_t* ids, void* stream) {
  if (!x || !vals || !ids) return blm_fail(BLM_ERR_INVALID, "blm_topk_rows: null operand");
  if (R < 0 || V <= 0 || ldx < V) return blm_fail(BLM_ERR_INVALID, "blm_topk_rows: bad shape");
  if (k < 1 || k > V || k > BLM_TOPK_MAX)
    return blm_fail(BLM_ERR_INVALID, "blm_topk_rows: k = %d outside [1, min(V, BLM_TOPK_MAX = %d)]", k, BLM_TOPK_MAX);
  if (!blm::extents_ok({R, (long)ldx})) return blm_fail(BLM_ERR_INVALID, "blm_topk_rows: extents too large");
  if (R == 0) return BLM_OK;
  hipLaunchKernelGGL(topk_rows_kernel, dim3(R), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, ldx, V, k, vals, ids);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_beam_select(const float* cand_vals, const int64_t* cand_ids, const float* score, const uint8_t* finished, int G,
                               int B, int k, int64_t eos, float* score_out, uint8_t* finished_out, int64_t* parent, int64_t* token,
                               void* stream) {
  if (!cand_vals || !cand_ids || !score || !finished || !score_out || !finished_out || !parent || !token)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select: null operand");
  if (G < 0 || B < 1 || k < 1) return blm_fail(BLM_ERR_INVALID, "blm_beam_select: bad shape");
  if (B > BLM_TOPK_MAX) return blm_fail(BLM_ERR_INVALID, "blm_beam_select: B = %d beams, BLM_TOPK_MAX is %d", B, BLM_TOPK_MAX);
  if (!blm::extents_ok({G, B, k}) || (long)B * k > blm::kMaxExtent)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select: extents too large");
  if (score == score_out || finished == finished_out)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select: the state before and after the step must be two buffers");
  if (G == 0) return BLM_OK;
  hipLaunchKernelGGL(beam_select_kernel, dim3(G), dim3(kThreads), 0, static_cast<hipStream_t>(stream), cand_vals, cand_ids, score,
                     finished, B, k, eos, score_out, finished_out, parent, token);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_beam_select_pool(const float* cand_vals, const int64_t* cand_ids, const float* score, const uint8_t* live, int G,
                                    int B, int k, int V, int64_t eos, int step, int len, int min_len, float inv_norm,
                                    float inv_norm_max, int flush, const blm_beam_pool* pool, float* score_out, uint8_t* live_out,
                                    int64_t* parent, int64_t* token, uint8_t* done_out, uint8_t* all_done, void* stream) {
  if (!cand_vals || !cand_ids || !score || !live || !pool || !score_out || !live_out || !parent || !token || !done_out || !all_done)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: null operand");
  if (pool->abi_version != BLM_ABI_VERSION)
    return blm_fail(BLM_ERR_ABI, "blm_beam_select_pool: blm_beam_pool.abi_version %u, library %u", pool->abi_version, BLM_ABI_VERSION);
  if (!pool->norm || !pool->raw || !pool->len || !pool->step || !pool->parent || !pool->finished || !pool->count || !pool->inserted)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: null pool array");
  if (G < 0 || B < 1 || k < 1 || V < 1) return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: bad shape");
  if (B > BLM_TOPK_MAX / 2)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: B = %d beams, 2 B exceeds BLM_TOPK_MAX = %d", B, BLM_TOPK_MAX);
  if (k < (2 * B < V ? 2 * B : V))
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: k = %d candidates per beam, min(2 B, V) = %d needed", k, 2 * B < V ? 2 * B : V);
  if (pool->P < 1 || pool->P > BLM_TOPK_MAX)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: P = %d pool slots outside [1, BLM_TOPK_MAX = %d]", pool->P, BLM_TOPK_MAX);
  if (!blm::extents_ok({G, B, k}) || !blm::extents_ok({G, pool->P}) || (long)B * k > blm::kMaxExtent)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: extents too large");
  if (step < 0 || len < 1 || min_len < 0) return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: step >= 0, len >= 1 and min_len >= 0 expected");
  if (!(inv_norm_max >= 0.f) || !(inv_norm >= inv_norm_max) || inv_norm > 3e38f)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: 0 <= inv_norm_max <= inv_norm < inf expected");
  if (score == score_out || live == live_out)
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: the state before and after the step must be two buffers");
  auto al = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
  if (!al(cand_vals, 4) || !al(score, 4) || !al(score_out, 4) || !al(pool->norm, 4) || !al(pool->raw, 4) || !al(pool->len, 4) ||
      !al(pool->step, 4) || !al(pool->count, 4) || !al(cand_ids, 8) || !al(parent, 8) || !al(token, 8) || !al(pool->parent, 8) ||
      !al(pool->inserted, 8))
    return blm_fail(BLM_ERR_INVALID, "blm_beam_select_pool: misaligned operand (4 bytes for float / int32, 8 for int64)");
  if (G == 0) return BLM_OK;
  hipLaunchKernelGGL(beam_select_pool_kernel, dim3(G), dim3(kThreads), 0, static_cast<hipStream_t>(stream), cand_vals, cand_ids, score,
                     live, B, k, eos, step, len, min_len, inv_norm, inv_norm_max, flush, *pool, score_out, live_out, parent, token,
                     done_out);
  BLM_HIP(hipGetLastError());
  hipLaunchKernelGGL(all_done_kernel, dim3(1), dim3(kThreads), 0, static_cast<hipStream_t>(stream), done_out, G, all_done);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_sample_rows_filtered(const float* x, int64_t ldx, int R, int V, float temperature, int top_k, float top_p,
                                        const blm_rng* rng, int64_t* out, void* stream) {
  if (!x || !out) return blm_fail(BLM_ERR_INVALID, "blm_sample_rows_filtered: null operand");
  if (R < 0 || V <= 0 || ldx < V || !(temperature >= 0.f) || temperature > 3e38f)
    return blm_fail(BLM_ERR_INVALID, "blm_sample_rows_filtered: bad shape or temperature");
  if (top_k < 0) return blm_fail(BLM_ERR_INVALID, "blm_sample_rows_filtered: top_k < 0 (0: no limit)");
  if (!(top_p > 0.f) || top_p > 1.f) return blm_fail(BLM_ERR_INVALID, "blm_sample_rows_filtered: top_p outside (0, 1]");
  if (temperature > 0.f && !rng) return blm_fail(BLM_ERR_INVALID, "blm_sample_rows_filtered: sampling needs rng");
  if (!blm::extents_ok({R, (long)ldx})) return blm_fail(BLM_ERR_INVALID, "blm_sample_rows_filtered: extents too large");
  if (R == 0) return BLM_OK;
  const blm_rng r = rng ? *rng : blm_rng{0, 0, 0};
  hipLaunchKernelGGL(sample_rows_filtered_kernel, dim3(R), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, ldx, V,
                     temperature > 0.f ? 1.0f / temperature : 0.f, temperature > 0.f ? 0 : 1, top_k, top_p, r, out);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
