// Incremental decoding (bayeslms_amd/incremental.py): causal attention of a few new query rows per stream over a key/value
// cache that outlives one forward call, the cache's append and beam gather, the embedding at per-stream positions, and the
// row-wise log-softmax / sampling of the decoder output.  All vector ALU: one query row per (stream, head) leaves no matrix shape
// to fill, and every kernel here is bound by the bytes it moves.
//
// Cache layout (one fp32 allocation per state): [layer][k|v][stream < n_cap][head][t < max_len][head_dim]; each (stream, head)
// owns a contiguous max_len x head_dim panel.  Past lengths are an (N,) int32 device array.
#include "blm_device.h"
#include "blm_host.h"

namespace {

constexpr int kCh = 64;       // keys per split-K chunk: one per lane of a wave in the softmax
constexpr int kRows = 16;     // query rows per workgroup
constexpr int kHdMax = 128;   // largest head size
constexpr int kThreads = 256;

struct DecP {
  const float* q;
  int64_t ldq;
  const float* kv;      // this layer: K panels, then V panels n_cap * nhead * max_len * hd floats later
  const int32_t* past;
  const int32_t* n_new; // may be NULL: every row is real
  float* out;
  float* ws;
  int Tq, N, n_cap, nhead, max_len, hd, nchunks;
  float scale;
};

__device__ __forceinline__ int rows_of(const DecP& p, int n) {
  return p.n_new ? min(max(p.n_new[n], 0), p.Tq) : p.Tq;
}

// Stage keys [key0, key0 + nkeys) of one panel into LDS rows of stride hd + 1 (odd: lane j of a wave reading element d of key j
// hits bank (j * (hd + 1) + d) mod 64, a different bank per lane).  Rows past nkeys are zero.  VEC: 16-byte loads.
template <bool VEC>
__device__ __forceinline__ void load_panel_regs(float (&r)[kCh * kHdMax / kThreads], const float* panel, int nkeys, int hd) {
  constexpr int W = VEC ? 4 : 1, IT = kCh * kHdMax / (kThreads * W);
  const int total = nkeys * hd / W;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = threadIdx.x + i * kThreads;
    if (VEC) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < total) v = reinterpret_cast<const float4*>(panel)[e];
      r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    } else {
      r[i] = e < total ? panel[e] : 0.f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void store_panel_lds(const float (&r)[kCh * kHdMax / kThreads], float* s, int nkeys, int hd) {
  constexpr int W = VEC ? 4 : 1, IT = kCh * kHdMax / (kThreads * W);
  const int total = nkeys * hd / W;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = threadIdx.x + i * kThreads;
    if (e < total) {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const int f = e * W + w, j = f / hd, d = f - j * hd;
        s[j * (hd + 1) + d] = r[W * i + w];
      }
    }
  }
}

// One workgroup per (key chunk, stream * head, block of 16 query rows): scores of the block's rows against the chunk's keys (one
// key per lane, one row per wave at a time), the chunk's softmax partials (max, sum) and P.V, all written to the workspace.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void attn_decode_part_kernel(DecP p) {
  const int c = blockIdx.x, nh = blockIdx.y, tb = blockIdx.z * kRows;
  const int n = nh / p.nhead, h = nh - n * p.nhead;
  const int nr = rows_of(p, n), past = max(p.past[n], 0);
  const int t_end = min(tb + kRows, nr);
  if (tb >= t_end) return;
  const int key0 = c * kCh;
  const int last = min(past + t_end - 1, p.max_len - 1);  // the last key any row of this block attends
  if (key0 > last) return;
  const int nkeys = min(kCh, last + 1 - key0), rows = t_end - tb, hd = p.hd;

  __shared__ float sQ[kRows * kHdMax];
  __shared__ float sKV[kCh * (kHdMax + 1)];
  __shared__ float sP[kRows * kCh];

  const size_t panel = (size_t)p.max_len * hd;
  const float* kp = p.kv + ((size_t)n * p.nhead + h) * panel + (size_t)key0 * hd;
  const float* vp = kp + (size_t)p.n_cap * p.nhead * panel;

  float r[kCh * kHdMax / kThreads];
  load_panel_regs<VEC>(r, kp, nkeys, hd);
  for (int e = threadIdx.x; e < rows * hd; e += kThreads) {
    const int t = e / hd, d = e - t * hd;
    sQ[t * kHdMax + d] = p.q[((size_t)(tb + t) * p.N + n) * p.ldq + (size_t)h * hd + d] * p.scale;
  }
  store_panel_lds<VEC>(r, sKV, nkeys, hd);
  __syncthreads();
  load_panel_regs<VEC>(r, vp, nkeys, hd);  // V in flight while the scores are computed

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* kr = sKV + lane * (hd + 1);
  float* ws_ml = p.ws;
  float* ws_acc = p.ws + 2 * (size_t)p.N * p.nhead * p.Tq * p.nchunks;
  for (int t = wv; t < rows; t += kThreads / 64) {
    const float* qr = sQ + t * kHdMax;
    float s = 0.f;
    for (int d = 0; d < hd; ++d) s = fmaf(qr[d], kr[d], s);
    const bool ok = lane < nkeys && key0 + lane <= past + tb + t;
    s = ok ? s : -INFINITY;
    const float m = blm::wave_max(s);
    const float e = ok ? __expf(s - m) : 0.f;
    const float l = blm::wave_sum(e);
    sP[t * kCh + lane] = e;
    if (lane == 0) {
      const size_t pi = (((size_t)n * p.nhead + h) * p.Tq + tb + t) * p.nchunks + c;
      ws_ml[2 * pi] = m;
      ws_ml[2 * pi + 1] = l;
    }
  }
  __syncthreads();
  store_panel_lds<VEC>(r, sKV, nkeys, hd);
  __syncthreads();
  for (int e = threadIdx.x; e < rows * hd; e += kThreads) {
    const int t = e / hd, d = e - t * hd;
    const float* pr = sP + t * kCh;
    float acc = 0.f;
    for (int j = 0; j < nkeys; ++j) acc = fmaf(pr[j], sKV[j * (hd + 1) + d], acc);
    const size_t pi = (((size_t)n * p.nhead + h) * p.Tq + tb + t) * p.nchunks + c;
    ws_acc[pi * hd + d] = acc;
  }
}

// One workgroup per (row, stream, head): the chunks' partials combined in chunk order (no atomics: bitwise repeatable).
__global__ __launch_bounds__(kHdMax) void attn_decode_combine_kernel(DecP p) {
  const int bid = blockIdx.x;
  const int t = bid / (p.N * p.nhead), rem = bid - t * p.N * p.nhead, n = rem / p.nhead, h = rem - n * p.nhead;
  const int d = threadIdx.x;
  if (d >= p.hd) return;
  float* o = p.out + ((size_t)t * p.N + n) * ((size_t)p.nhead * p.hd) + (size_t)h * p.hd + d;
  if (t >= rows_of(p, n)) {  // padding row of a ragged chunk
    *o = 0.f;
    return;
  }
  const int pos = min(max(p.past[n], 0) + t, p.max_len - 1);
  const int clast = min(pos / kCh, p.nchunks - 1);
  const size_t base = (((size_t)n * p.nhead + h) * p.Tq + t) * p.nchunks;
  const float* ml = p.ws + 2 * base;
  const float* acc = p.ws + 2 * (size_t)p.N * p.nhead * p.Tq * p.nchunks + base * p.hd + d;
  float M = -INFINITY;
  for (int c = 0; c <= clast; ++c) M = fmaxf(M, ml[2 * c]);
  float L = 0.f, A = 0.f;
  for (int c = 0; c <= clast; ++c) {
    const float w = ml[2 * c] == -INFINITY ? 0.f : __expf(ml[2 * c] - M);
    L = fmaf(ml[2 * c + 1], w, L);
    A = fmaf(acc[(size_t)c * p.hd], w, A);
  }
  *o = A / L;
}

__global__ __launch_bounds__(kThreads) void kv_append_kernel(const float* k, const float* v, int64_t ld, float* kv,
                                                             const int32_t* past, const int32_t* n_new, int Tq, int N, int n_cap,
                                                             int nhead, int max_len, int hd) {
  const int t = blockIdx.x / N, n = blockIdx.x - t * N;
  const int nr = n_new ? min(max(n_new[n], 0), Tq) : Tq;
  const int pos = max(past[n], 0) + t;
  if (t >= nr || pos >= max_len) return;
  const size_t panel = (size_t)max_len * hd, vofs = (size_t)n_cap * nhead * panel;
  const size_t src = ((size_t)t * N + n) * ld;
  for (int i = threadIdx.x; i < nhead * hd; i += kThreads) {
    const int h = i / hd, d = i - h * hd;
    const size_t dst = ((size_t)n * nhead + h) * panel + (size_t)pos * hd + d;
    kv[dst] = k[src + i];
    kv[vofs + dst] = v[src + i];
  }
}

constexpr int kGatherChunk = 4096;  // floats per workgroup of blm_kv_gather

template <bool VEC>
__global__ __launch_bounds__(kThreads) void kv_gather_kernel(const float* src, float* dst, const int64_t* idx, const int32_t* len,
                                                             int32_t* len_out, int M, int n_src, int n_cap, int nhead, int max_len,
                                                             int hd) {
  const int pnl = blockIdx.x;
  const int o = pnl / (M * nhead), r = pnl - o * M * nhead, j = r / nhead, h = r - j * nhead;
  const int64_t i = idx[j];
  const bool ok = i >= 0 && i < n_src;
  const int live = !ok ? 0 : (len ? min(max(len[i], 0), max_len) : max_len);
  if (len_out && o == 0 && h == 0 && blockIdx.y == 0 && threadIdx.x == 0) len_out[j] = live;
  if (!ok) return;
  const size_t panel = (size_t)max_len * hd;
  const float* s = src + (((size_t)o * n_cap + i) * nhead + h) * panel;
  float* dd = dst + (((size_t)o * n_cap + j) * nhead + h) * panel;
  const int64_t nf = (int64_t)live * hd, lo = (int64_t)blockIdx.y * kGatherChunk, hi = min(nf, lo + kGatherChunk);
  if (VEC) {
    for (int64_t e = lo + 4 * threadIdx.x; e < hi; e += 4 * kThreads)
      *reinterpret_cast<float4*>(dd + e) = *reinterpret_cast<const float4*>(s + e);
  } else {
    for (int64_t e = lo + threadIdx.x; e < hi; e += kThreads) dd[e] = s[e];
  }
}

__global__ __launch_bounds__(kThreads) void embed_at_kernel(const int64_t* ids, const float* enc, int64_t vocab, float scale,
                                                            const float* x, const float* pe, int pe_rows, const int32_t* pos0,
                                                            float* out, int N, int D) {
  const int row = blockIdx.x, t = row / N, n = row - t * N;
  const float* src = nullptr;
  bool bad = false;
  if (ids) {
    const int64_t id = ids[row];
    bad = id < 0 || id >= vocab;
    src = bad ? nullptr : enc + (size_t)id * D;
  } else {
    src = x + (size_t)row * D;
  }
  const float* pr = nullptr;
  if (pe) {
    const int64_t pos = (int64_t)pos0[n] + t;
    bad = bad || pos < 0 || pos >= pe_rows;
    pr = bad ? nullptr : pe + (size_t)pos * D;
  }
  float* o = out + (size_t)row * D;
  for (int d = threadIdx.x; d < D; d += kThreads) {
    if (bad) {
      o[d] = NAN;
      continue;
    }
    const float a = ids ? src[d] * scale : src[d];
    o[d] = pr ? a + pr[d] : a;
  }
}

__global__ __launch_bounds__(kThreads) void log_softmax_rows_kernel(const float* x, int64_t ldx, float* out, int64_t ldo, int V) {
  __shared__ float red[kThreads / 64];
  const float* xr = x + (size_t)blockIdx.x * ldx;
  float* orow = out + (size_t)blockIdx.x * ldo;
  float m = -INFINITY;
  for (int c = threadIdx.x; c < V; c += kThreads) m = fmaxf(m, xr[c]);
  m = blm::block_max<kThreads / 64>(m, red);
  float s = 0.f;
  for (int c = threadIdx.x; c < V; c += kThreads) s += __expf(xr[c] - m);
  s = blm::block_sum<kThreads / 64>(s, red);
  const float lse = m + logf(s);
  for (int c = threadIdx.x; c < V; c += kThreads) orow[c] = xr[c] - lse;
}

__global__ __launch_bounds__(kThreads) void sample_rows_kernel(const float* x, int64_t ldx, int V, float inv_t, int greedy,
                                                               blm_rng rng, int64_t* out) {
  __shared__ float sv[kThreads / 64];
  __shared__ int si[kThreads / 64];
  const int row = blockIdx.x;
  const float* xr = x + (size_t)row * ldx;
  blm::Best b = {-INFINITY, blm::kNone};
  for (int c = threadIdx.x; c < V; c += kThreads) {
    float s = xr[c];
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

int chunks_of(int ctx_max) { return (ctx_max + kCh - 1) / kCh; }

}  // namespace

extern "C" int64_t blm_attn_decode_ws_floats(int Tq, int N, int nhead, int ctx_max, int head_dim) {
  if (Tq < 0 || N < 0 || nhead <= 0 || ctx_max < 0 || head_dim <= 0 || head_dim > kHdMax) return 0;
  const long nc = chunks_of(ctx_max);
  if (!blm::extents_ok({Tq, N, nhead, nc, head_dim + 2})) return 0;
  return (int64_t)Tq * N * nhead * nc * (head_dim + 2);
}

extern "C" int blm_attn_decode(const float* q, int64_t ld_q, const float* kv, const int32_t* past, const int32_t* n_new, float* out,
                               float* ws, int64_t ws_floats, int Tq, int N, int n_cap, int nhead, int max_len, int head_dim,
                               int ctx_max, void* stream) {
  if (!q || !kv || !past || !out || !ws) return blm_fail(BLM_ERR_INVALID, "blm_attn_decode: null operand");
  if (Tq < 0 || N < 0 || n_cap < N || nhead <= 0 || head_dim <= 0 || max_len <= 0 || ctx_max < 0 || ctx_max > max_len)
    return blm_fail(BLM_ERR_INVALID, "blm_attn_decode: bad shape");
  if (head_dim > kHdMax) return blm_fail(BLM_ERR_UNSUPPORTED, "blm_attn_decode: head_dim %d not in 1..%d", head_dim, kHdMax);
  if (ld_q < (int64_t)nhead * head_dim) return blm_fail(BLM_ERR_INVALID, "blm_attn_decode: ld_q too small");
  if (!blm::extents_ok({Tq, N, (long)ld_q}) || !blm::extents_ok({2, n_cap, nhead, max_len, head_dim}) ||
      (long)N * nhead > 65535 || Tq > 65535 * kRows || (long)Tq * N * nhead > (1L << 31) - 1)
    return blm_fail(BLM_ERR_INVALID, "blm_attn_decode: extents too large");
  if (Tq == 0 || N == 0) return BLM_OK;
  if (ctx_max == 0) return blm_fail(BLM_ERR_INVALID, "blm_attn_decode: ctx_max 0 with rows to attend");
  const int64_t need = blm_attn_decode_ws_floats(Tq, N, nhead, ctx_max, head_dim);
  if (need <= 0 || ws_floats < need)
    return blm_fail(BLM_ERR_INVALID, "blm_attn_decode: workspace %lld floats < %lld", (long long)ws_floats, (long long)need);
  DecP p{q, ld_q, kv, past, n_new, out, ws, Tq, N, n_cap, nhead, max_len, head_dim, chunks_of(ctx_max),
         1.0f / sqrtf((float)head_dim)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(p.nchunks, N * nhead, (Tq + kRows - 1) / kRows);
  if (head_dim % 4 == 0 && blm::aligned16(kv))
    hipLaunchKernelGGL(attn_decode_part_kernel<true>, grid, dim3(kThreads), 0, st, p);
  else
    hipLaunchKernelGGL(attn_decode_part_kernel<false>, grid, dim3(kThreads), 0, st, p);
  BLM_HIP(hipGetLastError());
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)Tq * N * nhead), dim3(kHdMax), 0, st, p);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_kv_append(const float* k, const float* v, int64_t ld_kv, float* kv, const int32_t* past, const int32_t* n_new,
                             int Tq, int N, int n_cap, int nhead, int max_len, int head_dim, void* stream) {
  if (!k || !v || !kv || !past) return blm_fail(BLM_ERR_INVALID, "blm_kv_append: null operand");
  if (Tq < 0 || N < 0 || n_cap < N || nhead <= 0 || head_dim <= 0 || max_len <= 0 || ld_kv < (int64_t)nhead * head_dim)
    return blm_fail(BLM_ERR_INVALID, "blm_kv_append: bad shape");
  if (!blm::extents_ok({Tq, N, (long)ld_kv}) || !blm::extents_ok({2, n_cap, nhead, max_len, head_dim}) || (long)Tq * N > (1L << 31) - 1)
    return blm_fail(BLM_ERR_INVALID, "blm_kv_append: extents too large");
  if (Tq == 0 || N == 0) return BLM_OK;
  hipLaunchKernelGGL(kv_append_kernel, dim3((unsigned)Tq * N), dim3(kThreads), 0, static_cast<hipStream_t>(stream), k, v, ld_kv, kv,
                     past, n_new, Tq, N, n_cap, nhead, max_len, head_dim);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_kv_gather(const float* src, float* dst, const int64_t* idx, const int32_t* len, int32_t* len_out, int M, int n_src,
                             int n_cap, int outer, int nhead, int max_len, int head_dim, void* stream) {
  if (!src || !dst || !idx) return blm_fail(BLM_ERR_INVALID, "blm_kv_gather: null operand");
  if (M < 0 || n_src < 0 || n_cap < M || n_cap < n_src || outer <= 0 || nhead <= 0 || max_len <= 0 || head_dim <= 0)
    return blm_fail(BLM_ERR_INVALID, "blm_kv_gather: bad shape");
  if (!blm::extents_ok({outer, n_cap, nhead, max_len, head_dim}) || (long)outer * M * nhead > (1L << 31) - 1)
    return blm_fail(BLM_ERR_INVALID, "blm_kv_gather: extents too large");
  const uintptr_t bytes = (uintptr_t)outer * n_cap * nhead * max_len * head_dim * sizeof(float);
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  if (s0 < d0 + bytes && d0 < s0 + bytes)
    return blm_fail(BLM_ERR_INVALID, "blm_kv_gather: source and destination states overlap (double-buffer the state)");
  if (len && len_out && len == len_out) return blm_fail(BLM_ERR_INVALID, "blm_kv_gather: len and len_out alias");
  if (M == 0) return BLM_OK;
  const long panel = (long)max_len * head_dim;
  const dim3 grid((unsigned)(outer * M * nhead), (unsigned)((panel + kGatherChunk - 1) / kGatherChunk));
  if (grid.y > 65535) return blm_fail(BLM_ERR_INVALID, "blm_kv_gather: panel too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (head_dim % 4 == 0 && ((s0 | d0) & 15) == 0)
    hipLaunchKernelGGL(kv_gather_kernel<true>, grid, dim3(kThreads), 0, st, src, dst, idx, len, len_out, M, n_src, n_cap, nhead,
                       max_len, head_dim);
  else
    hipLaunchKernelGGL(kv_gather_kernel<false>, grid, dim3(kThreads), 0, st, src, dst, idx, len, len_out, M, n_src, n_cap, nhead,
                       max_len, head_dim);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_embed_at(const int64_t* ids, const float* enc, int64_t vocab, float scale, const float* x, const float* pe,
                            int pe_rows, const int32_t* pos0, float* out, int Tq, int N, int D, void* stream) {
  if (!out || (ids && !enc) || (!ids && !x) || (pe && !pos0)) return blm_fail(BLM_ERR_INVALID, "blm_embed_at: null operand");
  if (Tq < 0 || N < 0 || D <= 0 || (ids && vocab <= 0) || (pe && pe_rows <= 0)) return blm_fail(BLM_ERR_INVALID, "blm_embed_at: bad shape");
  if (!blm::extents_ok({Tq, N, D}) || (ids && !blm::extents_ok({(long)vocab, D})) || (pe && !blm::extents_ok({pe_rows, D})) ||
      (long)Tq * N > (1L << 31) - 1)
    return blm_fail(BLM_ERR_INVALID, "blm_embed_at: extents too large");
  if (Tq == 0 || N == 0) return BLM_OK;
  hipLaunchKernelGGL(embed_at_kernel, dim3((unsigned)Tq * N), dim3(kThreads), 0, static_cast<hipStream_t>(stream), ids, enc, vocab,
                     scale, x, pe, pe_rows, pos0, out, N, D);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_log_softmax_rows(const float* x, int64_t ldx, float* out, int64_t ldo, int R, int V, void* stream) {
  if (!x || !out) return blm_fail(BLM_ERR_INVALID, "blm_log_softmax_rows: null operand");
  if (R < 0 || V <= 0 || ldx < V || ldo < V) return blm_fail(BLM_ERR_INVALID, "blm_log_softmax_rows: bad shape");
  if (!blm::extents_ok({R, (long)ldx}) || !blm::extents_ok({R, (long)ldo}))
    return blm_fail(BLM_ERR_INVALID, "blm_log_softmax_rows: extents too large");
  if (x != out || ldx != ldo) {
    // exact in-place use (out == x, same row stride) or disjoint buffers: a partial overlap would race across rows
    const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(out);
    if (a < b + (uintptr_t)R * ldo * 4 && b < a + (uintptr_t)R * ldx * 4)
      return blm_fail(BLM_ERR_INVALID, "blm_log_softmax_rows: x and out overlap other than exactly in place");
  }
  if (R == 0) return BLM_OK;
  hipLaunchKernelGGL(log_softmax_rows_kernel, dim3(R), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, ldx, out, ldo, V);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}

extern "C" int blm_sample_rows(const float* x, int64_t ldx, int R, int V, float temperature, const blm_rng* rng, int64_t* out,
                               void* stream) {
  if (!x || !out) return blm_fail(BLM_ERR_INVALID, "blm_sample_rows: null operand");
  if (R < 0 || V <= 0 || ldx < V || !(temperature >= 0.f) || temperature > 3e38f)
    return blm_fail(BLM_ERR_INVALID, "blm_sample_rows: bad shape or temperature");
  if (temperature > 0.f && !rng) return blm_fail(BLM_ERR_INVALID, "blm_sample_rows: sampling needs rng");
  if (!blm::extents_ok({R, (long)ldx})) return blm_fail(BLM_ERR_INVALID, "blm_sample_rows: extents too large");
  if (R == 0) return BLM_OK;
  const blm_rng r = rng ? *rng : blm_rng{0, 0, 0};
  hipLaunchKernelGGL(sample_rows_kernel, dim3(R), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, ldx, V,
                     temperature > 0.f ? 1.0f / temperature : 0.f, temperature > 0.f ? 0 : 1, r, out);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
