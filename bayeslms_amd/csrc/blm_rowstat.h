// The online row statistics of a workgroup of TPB threads per row (rowstats.hip, laplace.hip), once: the target prologue, the
// walk over a row's columns, the fold of the lanes' states, the state family and the stores that finish a row.  A kernel picks
// a state, a column source and its vec / scalar form; the rules below are the same for all of them.  The trailing `p...` of every
// function is what a state's members need beside the state (the temperature list of RowAccT; nothing for the other two).
#pragma once
#include "blm_device.h"

namespace blm {

// ---------------------------------------------------------------- the target
struct RowTarget {
  bool has_t;
  int tg;    // the target's column, -1 without one
  float tv;  // its value as the source forms it; NaN without a target: NaN compares false, so nothing is counted
};
template <class Src>
__device__ __forceinline__ RowTarget row_target(const int64_t* tgt, int row, int V, const Src& src) {
  const int64_t t64 = tgt ? tgt[row] : -1;
  const bool has_t = t64 >= 0 && t64 < V;
  const int tg = has_t ? (int)t64 : -1;
  float aux;
  const float tv = has_t ? src.one(tg, aux) : NAN;
  return {has_t, tg, tv};
}

// ---------------------------------------------------------------- column sources
// one(c, aux) / quad(i, aux): the value of column c / of columns 4 i .. 4 i + 3 as the statistics see it, and in aux what the
// state's add() takes beside it (RowAccW: the column's variance; the other states ignore it)
struct RowCols {  // the row as it lies in memory
  const float* xr;
  __device__ __forceinline__ float one(int c, float& aux) const { return aux = xr[c]; }
  __device__ __forceinline__ float4 quad(int i, float4& aux) const { return aux = reinterpret_cast<const float4*>(xr)[i]; }
};

// ---------------------------------------------------------------- the states
// What the three states share, over their fields m (running max), am (its lowest index), cnt (rank count) and bad (NaN flag).
template <class S>
struct RowRules {
  // column c holds x.  NaN rule: a NaN (or, second form, a column the caller calls spoilt) marks the row.  Rank rule: a column
  // is ahead of the target when it is larger, or equal at a lower index; tv / tg: the target's value (NaN: no target) and index.
  __device__ __forceinline__ void note(float x, int c, float tv, int tg) {
    S& a = *static_cast<S*>(this);
    a.bad |= x != x;
    a.cnt += (x > tv || (x == tv && c < tg)) ? 1 : 0;
  }
  __device__ __forceinline__ void note(float x, int c, float tv, int tg, bool spoilt) {
    S& a = *static_cast<S*>(this);
    a.bad |= (x != x) || spoilt;
    a.cnt += (x > tv || (x == tv && c < tg)) ? 1 : 0;
  }
  // Tie rule: the lowest index wins a tie, whichever side it comes from.
  template <class... P>
  __device__ __forceinline__ void merge(const S& b, const P&... p) {
    S& a = *static_cast<S*>(this);
    const float M = fmaxf(a.m, b.m);
    if (b.m > a.m || (b.m == a.m && b.am < a.am)) a.am = b.am;  // before a.m moves
    S o = b;
    if (a.m < M) a.rescale(M, p...);
    if (o.m < M) o.rescale(M, p...);
    a.sum(o);
    a.cnt += b.cnt;
    a.bad |= b.bad;
  }
};

// s = sum exp(x - m), t = sum exp(x - m) (x - m) over the finite columns seen so far: log-sum-exp = m + log s and
// entropy = log s - t / s, both free of the cancellation that sum p x has for rows far from 0.
struct RowAcc : RowRules<RowAcc> {
  float m, s, t;
  int am, cnt, bad;
  // the state re-expressed for a max M > m (m == -inf: nothing summed yet, s = t = 0 stay)
  __device__ __forceinline__ void rescale(float M) {
    if (m > -INFINITY) {
      const float d = m - M, f = __expf(d);
      t = f * (t + d * s);
      s *= f;
    }
    m = M;
  }
  // column c, whose value does not exceed m
  __device__ __forceinline__ void add(float x, float, int c, float tv, int tg) {
    const float d = x - m, e = __expf(d);
    const bool fin = x > -INFINITY;  // false for NaN too
    s += fin ? e : 0.f;
    t += fin ? e * d : 0.f;  // p log p -> 0 at p = 0
    note(x, c, tv, tg);
  }
  __device__ __forceinline__ void sum(const RowAcc& o) {
    s += o.s;
    t += o.t;
  }
  __device__ __forceinline__ RowAcc shfl(int o) const {
    RowAcc b;
    b.m = __shfl_xor(m, o, 64);
    b.s = __shfl_xor(s, o, 64);
    b.t = __shfl_xor(t, o, 64);
    b.am = __shfl_xor(am, o, 64);
    b.cnt = __shfl_xor(cnt, o, 64);
    b.bad = __shfl_xor(bad, o, 64);
    return b;
  }
};

// RowAcc with one more sum: w = sum exp(y - m) var
struct RowAccW : RowRules<RowAccW> {
  float m, s, t, w;
  int am, cnt, bad;
  __device__ __forceinline__ void rescale(float M) {
    if (m > -INFINITY) {
      const float d = m - M, f = __expf(d);
      t = f * (t + d * s);
      s *= f;
      w *= f;
    }
    m = M;
  }
  __device__ __forceinline__ void add(float y, float var, int c, float tv, int tg) {
    const float d = y - m, e = __expf(d);
    const bool fin = y > -INFINITY;  // false for NaN too
    s += fin ? e : 0.f;
    t += fin ? e * d : 0.f;
    w += fin ? e * var : 0.f;
    note(y, c, tv, tg, !(var >= 0.f && var < INFINITY));
  }
  __device__ __forceinline__ void sum(const RowAccW& o) {
    s += o.s;
    t += o.t;
    w += o.w;
  }
  __device__ __forceinline__ RowAccW shfl(int o) const {
    RowAccW b;
    b.m = __shfl_xor(m, o, 64);
    b.s = __shfl_xor(s, o, 64);
    b.t = __shfl_xor(t, o, 64);
    b.w = __shfl_xor(w, o, 64);
    b.am = __shfl_xor(am, o, 64);
    b.cnt = __shfl_xor(cnt, o, 64);
    b.bad = __shfl_xor(bad, o, 64);
    return b;
  }
};

// J inverse temperatures b_j: s_j = sum exp(b_j d), u_j = sum exp(b_j d) d with d = x - m UNSCALED; m, am, cnt and bad do not
// depend on b > 0 and are carried once.  tp.b2[j] = float(b_j log2 e).  Fused multiply-adds are written out and contraction is
// off in every member (the pragma is lexical: it has to stand in each), so slot j runs the same operations whatever J is.
template <int J>
struct RowAccT : RowRules<RowAccT<J>> {
  float m;
  int am, cnt, bad;
  float s[J], u[J];
  // the state re-expressed for a max M > m (m == -inf: nothing summed yet, s = u = 0 stay)
  template <class TP>
  __device__ __forceinline__ void rescale(float M, const TP& tp) {
#pragma clang fp contract(off)
    if (m > -INFINITY) {
      const float d = m - M;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const float f = __builtin_amdgcn_exp2f(tp.b2[j] * d);
        u[j] = f * __builtin_fmaf(d, s[j], u[j]);
        s[j] = f * s[j];
      }
    }
    m = M;
  }
  template <class TP>
  __device__ __forceinline__ void add(float x, float, int c, float tv, int tg, const TP& tp) {
#pragma clang fp contract(off)
    const bool fin = x > -INFINITY;  // false for NaN too
    const float dx = x - m;
    const float de = fin ? dx : -INFINITY;  // b2 > 0: exp2(b2 * -inf) = 0, one select for all J instead of one each
    const float d = fin ? dx : 0.f;         // p log p -> 0 at p = 0
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float e = __builtin_amdgcn_exp2f(tp.b2[j] * de);
      s[j] += e;
      u[j] = __builtin_fmaf(e, d, u[j]);
    }
    this->note(x, c, tv, tg);
  }
  __device__ __forceinline__ void sum(const RowAccT& o) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < J; ++j) {
      s[j] += o.s[j];
      u[j] += o.u[j];
    }
  }
  __device__ __forceinline__ RowAccT shfl(int o) const {
    RowAccT b;
    b.m = __shfl_xor(m, o, 64);
    b.am = __shfl_xor(am, o, 64);
    b.cnt = __shfl_xor(cnt, o, 64);
    b.bad = __shfl_xor(bad, o, 64);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      b.s[j] = __shfl_xor(s[j], o, 64);
      b.u[j] = __shfl_xor(u[j], o, 64);
    }
    return b;
  }
};

// ---------------------------------------------------------------- the walk
// The quads take the state by value and return it, the columns update it behind a reference: the other way round either loop
// compiles to more instructions (six more in the float4 loop of the plain state, eight in the scalar loop at J = 8).
// one column: the max moves first (lowest index: a later equal column does not take it), then the column is summed
template <class S, class Src, class... P>
__device__ __forceinline__ void row_column(S& a, const Src& src, int c, const RowTarget& t, const P&... p) {
  float aux;
  const float v = src.one(c, aux);
  if (v > a.m) {
    a.rescale(v, p...);
    a.am = c;
  }
  a.add(v, aux, c, t.tv, t.tg, p...);
}
// columns c0, c0 + TPB, .. below V: a row on the scalar path (c0 = threadIdx.x), or the columns the quads leave
template <int TPB, class S, class Src, class... P>
__device__ __forceinline__ void row_columns(S& a, const Src& src, int c0, int V, const RowTarget& t, const P&... p) {
  for (int c = c0; c < V; c += TPB) row_column(a, src, c, t, p...);
}
// quads threadIdx.x, threadIdx.x + TPB, .. below n4, 16 bytes a load: the max of four, its lowest index, four adds
template <int TPB, class S, class Src, class... P>
__device__ __forceinline__ S row_quads(S a, const Src& src, int n4, const RowTarget& t, const P&... p) {
  for (int i = threadIdx.x; i < n4; i += TPB) {
    float4 aux;
    const float4 v = src.quad(i, aux);
    const int c = 4 * i;
    const float cm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (cm > a.m) {
      a.rescale(cm, p...);
      a.am = c + (v.x == cm ? 0 : (v.y == cm ? 1 : (v.z == cm ? 2 : 3)));
    }
    a.add(v.x, aux.x, c, t.tv, t.tg, p...);
    a.add(v.y, aux.y, c + 1, t.tv, t.tg, p...);
    a.add(v.z, aux.z, c + 2, t.tv, t.tg, p...);
    a.add(v.w, aux.w, c + 3, t.tv, t.tg, p...);
  }
  return a;
}
// the whole row with the form chosen at compile time
template <int TPB, bool VEC, class S, class Src, class... P>
__device__ __forceinline__ void row_walk(S& a, const Src& src, int V, const RowTarget& t, const P&... p) {
  if (VEC) {
    const int n4 = V >> 2;
    a = row_quads<TPB>(a, src, n4, t, p...);
    const int c = 4 * n4 + threadIdx.x;  // the V % 4 last columns
    if (c < V) row_column(a, src, c, t, p...);
  } else {
    row_columns<TPB>(a, src, threadIdx.x, V, t, p...);
  }
}

// ---------------------------------------------------------------- the fold
// The lanes' states into thread 0's, in a fixed order: xor butterfly inside a wave, then waves 1 .. TPB / 64 - 1 in turn through
// red (one state of LDS per wave).  True for thread 0, which holds the row's state; every other thread is done.
template <int TPB, class S, class... P>
__device__ __forceinline__ bool row_state_fold(S& a, S* red, const P&... p) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a.merge(a.shfl(o), p...);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = a;
  __syncthreads();
  if (threadIdx.x != 0) return false;
  for (int k = 1; k < TPB / 64; ++k) a.merge(red[k], p...);
  return true;
}

// ---------------------------------------------------------------- the finish
// Element o of the three float figures and the row's two indices; an array the caller left out is skipped.  A bad row is
// NaN / -1 throughout, a row without a target in nll and rank.
__device__ __forceinline__ void row_store_figures(size_t o, bool bad, bool has_t, float nll_v, float conf_v, float entropy_v,
                                                  float* nll, float* conf, float* entropy) {
  if (nll) nll[o] = (bad || !has_t) ? NAN : nll_v;
  if (conf) conf[o] = bad ? NAN : conf_v;
  if (entropy) entropy[o] = bad ? NAN : entropy_v;
}
__device__ __forceinline__ void row_store_indices(int row, bool bad, bool has_t, int am, int cnt, int32_t* pred, int32_t* rank) {
  if (pred) pred[row] = bad ? -1 : am;
  if (rank) rank[row] = (bad || !has_t) ? -1 : cnt;
}
// the five figures of a row from a state with one s and one t (RowAcc, RowAccW)
template <class S>
__device__ __forceinline__ void row_finish(int row, const S& a, const RowTarget& t, float* nll, float* conf, float* entropy,
                                           int32_t* pred, int32_t* rank) {
  const float ls = logf(a.s);
  const bool bad = a.bad != 0;
  row_store_figures(row, bad, t.has_t, (a.m - t.tv) + ls /* = lse - x[target] */, 1.0f / a.s /* = exp(max - lse) */,
                    ls - a.t / a.s, nll, conf, entropy);
  row_store_indices(row, bad, t.has_t, a.am, a.cnt, pred, rank);
}

}  // namespace blm
