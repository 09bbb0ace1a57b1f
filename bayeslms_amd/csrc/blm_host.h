// Host-side error plumbing of the C ABI: status codes + thread-local message.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bayeslm.h"

int blm_fail(int status, const char* fmt, ...);

#define BLM_HIP(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return blm_fail(BLM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Extent checks shared by the entry points (found by the host-side UBSan build, tests/test_sanitizer_cpu.py): a launcher's size
// arithmetic -- ceil divisions on int extents, products of three extents, byte counts -- must not overflow whatever the caller
// passes.  An entry point accepts extents in [0, 2^30] whose product is at most 2^40 elements (4 TB of fp32: far beyond the
// 288 GB of HBM), and says BLM_ERR_INVALID otherwise.
#include <initializer_list>
#include <type_traits>
namespace blm {
constexpr long kMaxExtent = 1L << 30, kMaxElems = 1L << 40;
inline bool extents_ok(std::initializer_list<long> dims) {
  long prod = 1;
  for (long d : dims) {
    if (d < 0 || d > kMaxExtent) return false;
    if (d > 1) {
      if (prod > kMaxElems / d) return false;
      prod *= d;
    }
  }
  return true;
}
// every pointer given is 16-byte aligned; a null pointer (an operand the call leaves out) counts as aligned
template <class... P>
inline bool aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & 15) == 0;
}
// f(std::integral_constant<int, J>) for the built slot count J of 1, 2, 4, 8 that holds `count` values (temperatures, thetas,
// draws): 1 -> 1, 2 -> 2, 3..4 -> 4, 5..8 -> 8.  The entry point has checked 1 <= count <= 8, with its own message.
template <class F>
inline void for_slots(int count, F&& f) {
  if (count == 1) f(std::integral_constant<int, 1>{});
  else if (count == 2) f(std::integral_constant<int, 2>{});
  else if (count <= 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 8>{});
}
// The bytes [first, last) that an (M, V) float matrix at row stride ld touches (M >= 1), and the two questions the entry points
// ask of them: do two matrices share a byte, and may a result d be written where an operand z is read -- only over z itself,
// element for element, or clear of it.
struct Span {
  uintptr_t first, last;
};
inline Span span_of(const void* p, long M, long ld, long V) {
  const uintptr_t first = reinterpret_cast<uintptr_t>(p);
  return {first, first + ((uintptr_t)(M - 1) * (uintptr_t)ld + (uintptr_t)V) * 4};
}
inline bool overlaps(const Span& a, const Span& b) { return a.first < b.last && b.first < a.last; }
inline bool in_place_or_disjoint(const Span& d, const Span& z) { return d.first == z.first || !overlaps(d, z); }
// blm_colsum2 with a factor on the sums (out and, if given, out2 alike): the guarded-loader route of blm_gemm's colsum_a, whose
// sums carry the call's alpha -- the only caller with scale != 1, and it passes no out2
int colsum_scaled(const float* x, int64_t ld, float* out, float* out2, int M, int N, int accumulate, float scale, void* stream);
}  // namespace blm

// Kernel-selection options (blm_set_option / blm_get_option, include/bayeslm.h): every switch that picks between two BUILT
// forms of a kernel lives here -- one registry, settable at run time (so the GPU tests run both forms in one process), each
// initialised from its BLM_* environment variable on first use.  INTEGRATION.md lists them with the test that covers each.
namespace blm {
enum Opt { OPT_ATTN_HPW = 0, OPT_ATTN_SHORT, OPT_ATTN_VALU, OPT_LSTM_GEMV, OPT_LSTM_PIPE, OPT_LSTM_TAIL, OPT_DETERMINISTIC, OPT_LSTM_MB2, OPT_EDIT_LANE_MAX, OPT_COUNT };
int option(Opt o);
}  // namespace blm
