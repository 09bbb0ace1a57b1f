// Speculative sampling, the verification step (blm_spec_accept; definitions: include/bayeslm.h): G drafted words per stream
// against the target's G + 1 rows.  No row depends on another, so ONE launch of (G + 1) N workgroups computes every row's
// accept flag and the word it would emit -- the residual draw from max(p - q, 0) for t < G, the plain draw from p for the bonus
// row t = G -- whether or not an earlier position of its stream rejected; a second, small launch walks each stream's G flags.
// Rows behind a rejection are wasted work; what that buys is one pass instead of a chain per stream.
// Per row: max of both rows (one barrier pair), sum exp of both (one more), then one sweep that forms log p, log q, log rho and
// the Gumbel keys and reduces two arg-maxima (the residual draw, and the plain draw that stands in when no column has
// rho > 0) by blm_sample_rows' rule (blm_device.h's Best).  No atomics, fixed order: the same bits from every run.
#include <cmath>

#include "blm_device.h"
#include "blm_host.h"

namespace blm {
namespace {

constexpr int SPEC_TPB = 1024;  // 16 waves

// The Philox state of a row that no column changes: the ten round keys and the counter words (row, stream, step).  Formed once
// at the top of the kernel, outside every branch that depends on the thread, and pinned to scalar registers: left to the
// compiler the keys are formed inside the first such branch that draws, merged behind it, and then live in 40 vector
// registers, which the register-held rows do not leave.
struct SpecRng {
  uint32_t k0[10], k1[10], row, stream, step;
};
__device__ __forceinline__ SpecRng spec_rng(const blm_rng& rng, unsigned row) {
  SpecRng r;
  uint32_t k0 = (uint32_t)rng.seed, k1 = (uint32_t)(rng.seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    r.k0[i] = __builtin_amdgcn_readfirstlane(k0);
    r.k1[i] = __builtin_amdgcn_readfirstlane(k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r.row = __builtin_amdgcn_readfirstlane(row);
  r.stream = __builtin_amdgcn_readfirstlane(rng.stream);
  r.step = __builtin_amdgcn_readfirstlane(rng.step);
  return r;
}
// blm_sample_rows' uniform of the first Philox word at counter (col, row, stream, step): blm::philox4x32_10's rounds
// (blm_device.h) with the keys above
__device__ __forceinline__ float philox_u(unsigned col, const SpecRng& g) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  uint32_t c0 = col, c1 = g.row, c2 = g.stream, c3 = g.step;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ g.k0[r], n2 = hi0 ^ c3 ^ g.k1[r];
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
  }
  return ((float)(c0 >> 8) + 0.5f) * 5.9604644775390625e-08f;  // (0, 1)
}

struct SpecRow {  // a row's constants of the sweep, the same in every lane
  float beta, mp, lsp, mq, lsq;  // log p = beta (P - mp) - lsp,  log q = beta (Q - mq) - lsq: the accept rule
  float cp, cq;                  // beta mp + lsp, beta mq + lsq: log p = beta P - cp, log q = beta Q - cq in the sweep
};

// One column of the sweep.  The plain key is blm_sample_rows' own expression, so that it rounds as it does there.
// log p and log q are formed here as fma(beta, P, -cp) and fma(beta, Q, -cq), not from beta (P - mp): that product is what the
// sum before the sweep exponentiates, and the compiler keeps one per column alive across the barrier beside the row itself (the
// 9-quad form then spills 180 bytes per lane).  The two forms differ by the rounding of beta P, 4e-6 at |beta P| < 64.  Both logs
// by the SAME operations: a draft row equal to the target's bit for bit gives log q = log p bit for bit, rho = 0 in every column.
__device__ __forceinline__ void spec_elem(float pv, float qv, unsigned col, const SpecRow& c, const SpecRng& rng,
                                          Best& plain, Best& resid) {
  const float gn = logf(-logf(philox_u(col, rng)));  // -g
  float s = pv;
  s = s * c.beta - gn;
  best_of(plain, s, (int)col);
  // log rho = log p + log(1 - q / p): one exp and one log, and no underflow of p or q on the way
  const float lp = __builtin_fmaf(c.beta, pv, -c.cp), lq = __builtin_fmaf(c.beta, qv, -c.cq);
  const float r = 1.f - __expf(lq - lp);  // NaN when both are -inf, -inf when p = 0 < q
  if (r > 0.f) best_of(resid, (lp + __logf(r)) - gn, (int)col);
}

// what the first thread does with the reduced row: the accept flag and the candidate
// (it loads the drafted id and the two values at it only now: one thread, three words -- held from the top of the kernel they
// would cost every thread registers that the register-held rows do not leave)
__device__ __forceinline__ void spec_finish(unsigned row, bool bonus, bool bad, const float* x, const float* y,
                                            const int64_t* __restrict__ draft, int V, const SpecRow& c, const SpecRng& rng,
                                            const Best& plain, const Best& resid, uint8_t* __restrict__ accept,
                                            int64_t* __restrict__ cand) {
  const int pl = plain.i == kNone ? 0 : plain.i;
  if (bonus) {
    cand[row] = bad ? -1 : pl;
    return;
  }
  const long xd = draft[row];
  const bool valid = xd >= 0 && xd < V;
  const float px = valid ? x[xd] : 0.f, qx = valid ? y[xd] : 0.f;
  const float lpx = c.beta * (px - c.mp) - c.lsp, lqx = c.beta * (qx - c.mq) - c.lsq;
  const bool ok = !bad && valid && lqx > -INFINITY;
  accept[row] = ok && logf(philox_u(0xFFFFFFFFu, rng)) < fminf(0.f, lpx - lqx) ? 1 : 0;
  cand[row] = bad ? -1 : (resid.i == kNone ? pl : resid.i);
}

// Both rows held in registers, as ce_soft_row_kernel (distill.hip) holds them: 1024 threads x NV float4 of each cover
// V <= 4096 NV, every row is read from memory once, all 2 NV loads of a thread issued back to back.  Requires V >= 4, ldp and
// ldq multiples of 4 and 16-byte aligned bases (blm_spec_accept selects).  A bonus row (t = G) has no draft row: it reads its
// own P row in Q's place, so that rho = 0 in every column, and its candidate is the plain draw.
template <int NV>
__global__ __launch_bounds__(SPEC_TPB) void spec_row_kernel(const float* __restrict__ P, long ldp, const float* __restrict__ Q, long ldq,
                                                            const int64_t* __restrict__ draft, int GN, int V, float beta, blm_rng rng,
                                                            uint8_t* __restrict__ accept, int64_t* __restrict__ cand) {
  __shared__ float red[2][16];
  __shared__ float sv[2][16];
  __shared__ int si[2][16];
  const unsigned row = blockIdx.x;
  const bool bonus = row >= (unsigned)GN;
  const SpecRng g = spec_rng(rng, row);
  const float* x = P + (long)row * ldp;
  const float* y = bonus ? x : Q + (long)row * ldq;
  const unsigned t0 = threadIdx.x * 4u, Vu = (unsigned)V;  // unsigned: base + 32-bit offset addressing
  // whole quads only; a quad outside the row reads quad 0 (V >= 4) and is skipped wherever the quads are used.  The V % 4
  // columns behind the last whole quad are one extra (P, Q) pair in threads 0 .. V % 4 - 1.
  float4 v[NV], u[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const unsigned j = t0 + 4096u * i;
    const unsigned js = j + 3 < Vu ? j : 0u;
    v[i] = *reinterpret_cast<const float4*>(x + js);
    u[i] = *reinterpret_cast<const float4*>(y + js);
  }
  const unsigned je = (Vu & ~3u) + threadIdx.x;
  const bool extra = je < Vu;
  const float ze = extra ? x[je] : -INFINITY, le = extra ? y[je] : -INFINITY;
  float mp = ze, mq = le;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    mp = fmaxf(mp, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
    mq = fmaxf(mq, fmaxf(fmaxf(u[i].x, u[i].y), fmaxf(u[i].z, u[i].w)));
  }
  row_fold<ROW_MAX, ROW_UNIFORM>(red, mp, mq);
  // a NaN anywhere in a row makes its sum NaN (fmaxf skips it, exp does not); so does a row without a finite maximum
  float sp = extra ? __expf(beta * (ze - mp)) : 0.f, sq = extra ? __expf(beta * (le - mq)) : 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (!(t0 + 4096u * i + 3 < Vu)) continue;
    sp += (__expf(beta * (v[i].x - mp)) + __expf(beta * (v[i].y - mp))) + (__expf(beta * (v[i].z - mp)) + __expf(beta * (v[i].w - mp)));
    sq += (__expf(beta * (u[i].x - mq)) + __expf(beta * (u[i].y - mq))) + (__expf(beta * (u[i].z - mq)) + __expf(beta * (u[i].w - mq)));
  }
  row_fold<ROW_SUM, ROW_UNIFORM>(red, sp, sq);
  const bool bad = !(sp == sp) || !(sq == sq);
  const float lsp = __logf(sp), lsq = __logf(sq);
  const SpecRow c = {beta, mp, lsp, mq, lsq, beta * mp + lsp, beta * mq + lsq};
  Best plain = {-INFINITY, kNone}, resid = {-INFINITY, kNone};
  {
    if (extra) spec_elem(ze, le, je, c, g, plain, resid);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const unsigned j = t0 + 4096u * i;
      if (!(j + 3 < Vu)) continue;
      spec_elem(v[i].x, u[i].x, j, c, g, plain, resid);
      spec_elem(v[i].y, u[i].y, j + 1, c, g, plain, resid);
      spec_elem(v[i].z, u[i].z, j + 2, c, g, plain, resid);
      spec_elem(v[i].w, u[i].w, j + 3, c, g, plain, resid);
    }
  }
  block_best2<SPEC_TPB / 64>(plain, resid, sv, si);
  if (threadIdx.x == 0) spec_finish(row, bonus, bad, x, y, draft, V, c, g, plain, resid, accept, cand);
}

// Any V, any stride, any alignment: the rows are read twice, column by column -- an online (max, sum exp) sweep over both,
// then the key sweep (from L2 / the Infinity Cache where the rows still are).
__global__ __launch_bounds__(SPEC_TPB) void spec_sweep_kernel(const float* __restrict__ P, long ldp, const float* __restrict__ Q, long ldq,
                                                              const int64_t* __restrict__ draft, int GN, int V, float beta, blm_rng rng,
                                                              uint8_t* __restrict__ accept, int64_t* __restrict__ cand) {
  __shared__ float red[2][16];
  __shared__ float sv[2][16];
  __shared__ int si[2][16];
  const unsigned row = blockIdx.x;
  const bool bonus = row >= (unsigned)GN;
  const SpecRng g = spec_rng(rng, row);
  const float* x = P + (long)row * ldp;
  const float* y = bonus ? x : Q + (long)row * ldq;
  float tp = -INFINITY, tq = -INFINITY, sp = 0.f, sq = 0.f;  // this thread's running maxima and the sums under them
  for (int j = threadIdx.x; j < V; j += SPEC_TPB) {
    const float a = x[j], b = y[j];
    if (a > tp) { sp *= __expf(beta * (tp - a)); tp = a; }
    if (b > tq) { sq *= __expf(beta * (tq - b)); tq = b; }
    sp += tp > -INFINITY || a != a ? __expf(beta * (a - tp)) : 0.f;  // a NaN goes into the sum, a -inf under a -inf maximum does not
    sq += tq > -INFINITY || b != b ? __expf(beta * (b - tq)) : 0.f;
  }
  float mp = tp, mq = tq;
  row_fold<ROW_MAX, ROW_UNIFORM>(red, mp, mq);
  // a thread whose columns were all -inf holds a zero sum; a row whose every column is -inf has no finite maximum: NaN, as above
  sp = tp > -INFINITY ? sp * __expf(beta * (tp - mp)) : (mp > -INFINITY ? sp : NAN);
  sq = tq > -INFINITY ? sq * __expf(beta * (tq - mq)) : (mq > -INFINITY ? sq : NAN);
  row_fold<ROW_SUM, ROW_UNIFORM>(red, sp, sq);
  const bool bad = !(sp == sp) || !(sq == sq);
  const float lsp = __logf(sp), lsq = __logf(sq);
  const SpecRow c = {beta, mp, lsp, mq, lsq, beta * mp + lsp, beta * mq + lsq};
  Best plain = {-INFINITY, kNone}, resid = {-INFINITY, kNone};
  for (int j = threadIdx.x; j < V; j += SPEC_TPB) spec_elem(x[j], y[j], (unsigned)j, c, g, plain, resid);
  block_best2<SPEC_TPB / 64>(plain, resid, sv, si);
  if (threadIdx.x == 0) spec_finish(row, bonus, bad, x, y, draft, V, c, g, plain, resid, accept, cand);
}

// temperature 0: one read of P's row, the lowest index that holds its maximum; a NaN in the row spoils it
__global__ __launch_bounds__(SPEC_TPB) void spec_greedy_kernel(const float* __restrict__ P, long ldp, const int64_t* __restrict__ draft,
                                                               int GN, int V, uint8_t* __restrict__ accept, int64_t* __restrict__ cand) {
  __shared__ float sv[16];
  __shared__ int si[16];
  __shared__ int sn[16];
  const unsigned row = blockIdx.x;
  const float* x = P + (long)row * ldp;
  Best b = {-INFINITY, kNone};
  int nan = 0;
  for (int j = threadIdx.x; j < V; j += SPEC_TPB) {
    const float a = x[j];
    nan |= a != a;
    best_of(b, a, j);
  }
  block_best<SPEC_TPB / 64>(b, sv, si, &nan, sn);
  if (threadIdx.x == 0) {
    const long best = nan ? -1 : (b.i == kNone ? 0 : b.i);
    cand[row] = best;
    if (row < (unsigned)GN) accept[row] = !nan && draft[row] == best ? 1 : 0;
  }
}

// a thread per stream walks its G flags
__global__ __launch_bounds__(256) void spec_finish_kernel(const uint8_t* __restrict__ accept, const int64_t* __restrict__ cand, int G,
                                                          int N, int32_t* __restrict__ n_acc, int64_t* __restrict__ token) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  int t = 0;
  while (t < G && accept[(long)t * N + n]) ++t;
  n_acc[n] = t;
  token[n] = cand[(long)t * N + n];
}

bool overlap(const void* a, uintptr_t an, const void* b, uintptr_t bn) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a && b && a0 < b0 + bn && b0 < a0 + an;
}

}  // namespace
}  // namespace blm

using namespace blm;

extern "C" int blm_spec_accept(const float* p, int64_t ldp, const float* q, int64_t ldq, const int64_t* draft, int G, int N, int V,
                               float temperature, const blm_rng* rng, uint8_t* accept, int64_t* cand, int32_t* n_acc, int64_t* token,
                               void* stream) {
  if (!(temperature >= 0.f) || !std::isfinite(temperature))
    return blm_fail(BLM_ERR_INVALID, "blm_spec_accept: temperature = %g: a finite value >= 0 expected", (double)temperature);
  const bool greedy = temperature == 0.f;
  const float beta = greedy ? 0.f : 1.0f / temperature;
  if (!std::isfinite(beta)) return blm_fail(BLM_ERR_INVALID, "blm_spec_accept: 1 / temperature (%g) is no finite float32", (double)temperature);
  const char* missing = !p ? "p" : !draft ? "draft" : !accept ? "accept" : !cand ? "cand" : !n_acc ? "n_acc" : !token ? "token"
                        : (!greedy && !q) ? "q" : (!greedy && !rng) ? "rng" : nullptr;
  if (missing) return blm_fail(BLM_ERR_INVALID, "blm_spec_accept: %s is NULL (q and rng may be NULL at temperature 0 only)", missing);
  if (G < 1 || N < 1 || V <= 0) return blm_fail(BLM_ERR_INVALID, "blm_spec_accept: G = %d, N = %d, V = %d: G >= 1, N >= 1 and V > 0 expected", G, N, V);
  if (ldp < V || (q && ldq < V))
    return blm_fail(BLM_ERR_INVALID, "blm_spec_accept: row strides ldp = %lld, ldq = %lld must be >= V = %d", (long long)ldp, (long long)ldq, V);
  if (!extents_ok({(long)G + 1, N, (long)ldp}) || (q && !extents_ok({G, N, (long)ldq})) || ((long)G + 1) * N > (1L << 31) - 1)
    return blm_fail(BLM_ERR_INVALID, "blm_spec_accept: extents too large");
  const uintptr_t GN = (uintptr_t)G * N, RN = GN + N;
  const struct { const void* ptr; uintptr_t bytes; const char* name; } in[3] = {
      {p, ((RN - 1) * (uintptr_t)ldp + V) * 4, "p"}, {q, q ? ((GN - 1) * (uintptr_t)ldq + V) * 4 : 0, "q"}, {draft, GN * 8, "draft"}},
    out[4] = {{accept, GN, "accept"}, {cand, RN * 8, "cand"}, {n_acc, (uintptr_t)N * 4, "n_acc"}, {token, (uintptr_t)N * 8, "token"}};
  for (const auto& o : out)
    for (const auto& i : in)
      if (overlap(o.ptr, o.bytes, i.ptr, i.bytes)) return blm_fail(BLM_ERR_INVALID, "blm_spec_accept: %s overlaps %s", o.name, i.name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)RN), block(SPEC_TPB);
  if (greedy) {
    hipLaunchKernelGGL(spec_greedy_kernel, grid, block, 0, st, p, (long)ldp, draft, (int)GN, V, accept, cand);
  } else {
    const bool vec = ((ldp & 3) == 0) && ((ldq & 3) == 0) && aligned16(p, q);
    if (vec && V >= 4 && V <= 4096 * 3)
      hipLaunchKernelGGL(spec_row_kernel<3>, grid, block, 0, st, p, (long)ldp, q, (long)ldq, draft, (int)GN, V, beta, *rng, accept, cand);
    else if (vec && V >= 4 && V <= 4096 * 9)
      hipLaunchKernelGGL(spec_row_kernel<9>, grid, block, 0, st, p, (long)ldp, q, (long)ldq, draft, (int)GN, V, beta, *rng, accept, cand);
    else
      hipLaunchKernelGGL(spec_sweep_kernel, grid, block, 0, st, p, (long)ldp, q, (long)ldq, draft, (int)GN, V, beta, *rng, accept, cand);
  }
  BLM_HIP(hipGetLastError());
  hipLaunchKernelGGL(spec_finish_kernel, dim3((N + 255) / 256), dim3(256), 0, st, accept, cand, G, N, n_acc, token);
  BLM_HIP(hipGetLastError());
  return BLM_OK;
}
