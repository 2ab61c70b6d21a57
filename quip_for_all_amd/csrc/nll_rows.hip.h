// Scoring tail of a prompt pass (part of decode_glue.hip's translation unit; it joins the family of argmax_step_kernel): for
// every row of (rows, n) fp16 logits the log-sum-exp, the log-probability of the row's target token and the arg-max, one
// launch, no fp32 copy of the logits.  One workgroup of 1024 threads per row.
//
// Mapping: the row is cut into groups of eight consecutive logits, group g = elements [8 g, 8 g + 8); group g belongs to
// thread g mod 1024 (element i -> thread (i / 8) mod 1024, argmax_step_kernel's rule).  A group is ONE 16-byte load where
// the row starts on a 16-byte boundary and the group is whole, eight 2-byte loads otherwise (rows of an odd n, the tail);
// elements at or past n read as -inf.  Either way the thread holds the same eight values, so what a thread computes does
// not depend on the row's alignment or on `rows`: row r of a (rows, n) call has the bits of a (1, n) call on that row.
//
// Two passes over the row: (1) maximum and its first index (larger value, then lower index: torch.argmax's tie rule),
// (2) sum of exp(x - max) in fp32.  A thread keeps its first KEEP groups in registers between the passes and reads later
// groups a second time: KEEP = 4 holds a whole row up to n = 32768 (Llama-2; 50 registers, two rows per CU), KEEP = 8
// the first 65536 logits of a longer one (82 registers; 16 groups would hold Llama-3's row and spill).  The order of
// the sum is fixed: a thread adds its groups in order and the eight terms of a group in order, the 64 lanes of a wave
// meet in a butterfly, thread 0 adds the 16 wave sums in order.  LDS: the 16 partials of each reduction.  No scratch,
// no atomics; the results of a row are plain stores from thread 0.
//
// Rules (torch.logsumexp(x.float(), -1) and the subtraction, except where noted):
//   lse     = log(sum exp(x - m)) + m, m the row's maximum, or 0 where the maximum is not finite (then a NaN in the
//             row gives NaN, a +inf gives +inf, a row of all -inf gives -inf)
//   logprob = x[target] - lse;  target < 0: exactly 0 ("not scored");  target >= n: NaN, nothing is read;
//             lse not finite: NaN (torch's subtraction gives -inf for a finite target beside a +inf logit; a row whose
//             log-sum-exp is not a number has no usable score, so it is NaN for every target)
//   argmax  = first index of the largest logit; a row without one (all NaN / all -inf) gives 0 (argmax_step_kernel)
// Error bound of lse against float64 on the same fp16 logits: a thread adds at most ceil(n / 8192) * 8 positive terms
// serially (152 at n = 152064), the trees add 6 + 15 roundings, and a term that matters (x - m > -30) is off by at most
// 32 units of 2^-24 (one rounding of the difference, |x - m| 2^-24, carried through exp, plus expf's own unit): relative
// error of the sum < 205 * 2^-24 = 1.3e-5, which is the absolute error of its logarithm.
#pragma once
#include "launch.hip.h"
#include "quip_device.hip.h"

namespace quip {
namespace {

constexpr int kNllThreads = 1024;

// group g of the row as eight packed fp16 values; elements at or past n are -inf (0xfc00)
__device__ __forceinline__ uint4 nll_load8(const f16* __restrict__ row, int g, int n, bool vec) {
  const int i = g * 8;
  if (vec && i + 8 <= n) return *reinterpret_cast<const uint4*>(row + i);
  const unsigned short* raw = reinterpret_cast<const unsigned short*>(row);
  unsigned w[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const unsigned lo = i + 2 * p < n ? raw[i + 2 * p] : 0xfc00u;
    const unsigned hi = i + 2 * p + 1 < n ? raw[i + 2 * p + 1] : 0xfc00u;
    w[p] = lo | (hi << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void nll_scan8(const uint4& q, int i, float& best, int& bi) {
  const f16* h = reinterpret_cast<const f16*>(&q);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = (float)h[j];
    if (v > best || (v == best && i + j < bi)) { best = v; bi = i + j; }
  }
}

__device__ __forceinline__ float nll_sum8(const uint4& q, float off, float s) {
  const f16* h = reinterpret_cast<const f16*>(&q);
#pragma unroll
  for (int j = 0; j < 8; ++j) s += expf((float)h[j] - off);
  return s;
}

template <int KEEP>
__global__ __launch_bounds__(kNllThreads) void nll_rows_kernel(const f16* __restrict__ logits, int n,
                                                               const int64_t* __restrict__ target,
                                                               float* __restrict__ logprob, float* __restrict__ lse,
                                                               int64_t* __restrict__ argmax) {
  __shared__ float sv[16];
  __shared__ int si[16];
  __shared__ float ss[16];
  const int tid = threadIdx.x;
  const f16* row = logits + (size_t)blockIdx.x * n;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int groups = (n + 7) >> 3;
  const unsigned ninf2 = 0xfc00fc00u;

  // pass 1: maximum and its first index
  uint4 keep[KEEP];
  float best = -3.0e38f;
  int bi = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < KEEP; ++k) {
    const int g = tid + kNllThreads * k;
    keep[k] = g < groups ? nll_load8(row, g, n, vec) : make_uint4(ninf2, ninf2, ninf2, ninf2);
  }
#pragma unroll
  for (int k = 0; k < KEEP; ++k) nll_scan8(keep[k], (tid + kNllThreads * k) * 8, best, bi);
  for (int g = tid + kNllThreads * KEEP; g < groups; g += kNllThreads) nll_scan8(nll_load8(row, g, n, vec), g * 8, best, bi);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w)      // every thread, the same order: no second barrier for a broadcast
    if (w != (tid >> 6) && (sv[w] > best || (sv[w] == best && si[w] < bi))) { best = sv[w]; bi = si[w]; }
  // (bi >= n: no logit compared greater than the start value -- all NaN / all -inf; a +inf maximum sums around 0 too)
  const float m = bi < n ? best : -INFINITY;
  const float off = (m == INFINITY || m == -INFINITY) ? 0.f : m;

  // pass 2: sum of exp(x - off); padding (-inf) adds exact zeros
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < KEEP; ++k) s = nll_sum8(keep[k], off, s);
  for (int g = tid + kNllThreads * KEEP; g < groups; g += kNllThreads) s = nll_sum8(nll_load8(row, g, n, vec), off, s);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) ss[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    float tot = ss[0];
    for (int w = 1; w < 16; ++w) tot += ss[w];
    const float l = logf(tot) + off;
    const int64_t t = target[blockIdx.x];
    float lp = 0.f;
    if (t >= 0) {
      const bool finite = l == l && l != INFINITY && l != -INFINITY;
      lp = (t < n && finite) ? (float)row[t] - l : __builtin_nanf("");
    }
    logprob[blockIdx.x] = lp;
    if (lse) lse[blockIdx.x] = l;
    if (argmax) argmax[blockIdx.x] = bi < n ? bi : 0;
  }
}
}  // namespace

int nll_rows_launch(const void* logits, int rows, int n, const int64_t* target, float* logprob, float* lse,
                    int64_t* argmax, hipStream_t stream) {
  if (rows < 1 || n < 1 || n > (1 << 30)) return QUIP_ERR_BAD_SHAPE;      // (8 * group index stays an int)
  const f16* x = reinterpret_cast<const f16*>(logits);
  if (n <= 8 * kNllThreads * 4)
    return launch<nll_rows_kernel<4>>(dim3(rows), dim3(kNllThreads), 0, stream, x, n, target, logprob, lse, argmax);
  return launch<nll_rows_kernel<8>>(dim3(rows), dim3(kNllThreads), 0, stream, x, n, target, logprob, lse, argmax);
}

}  // namespace quip
