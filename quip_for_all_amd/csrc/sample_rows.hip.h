// Sampling tail of the decode step (part of decode_glue.hip's translation unit, beside argmax_step_kernel and
// nll_rows.hip.h): one token per row of (rows, n) fp16 logits, every row with its own temperature, top-k, top-p and seed,
// one launch.  One workgroup of 1024 threads per row.  The token is a deterministic function of (the row's bits, T, k, p,
// seed, pos): integer arithmetic from the weights on, so it does not depend on the order in which anything is added.
//
// Mapping (nll_rows.hip.h's): the row is cut into groups of eight consecutive logits, group g = elements [8 g, 8 g + 8),
// group g belongs to thread g mod 1024.  A group is ONE 16-byte load where the row starts on a 16-byte boundary and the
// group is whole, eight 2-byte loads otherwise (rows of an odd n, the tail); elements at or past n read as -inf.  Either
// way a thread holds the same eight values, and what is done with them commutes (integer atomics), so row r of a
// (rows, n) call has the bits of a (1, n) call on that row, aligned or not.
//
// Rules (DESIGN 4.16 has them in full; c = pos[r] before it is advanced):
//   greedy row   T is not > 0, or the row's maximum is not finite: token = first index of the largest logit, a row with
//                none gives 0 (argmax_step_kernel, bit for bit); kept = 1
//   classes      the distinct finite fp16 values v_1 > v_2 > ... (-0 is +0), multiplicities c_j; NaN and -inf carry no
//                mass; w_j = exp((v_j - v_1) / T); canonical order: classes descending, inside a class ascending index
//   top-k        1 <= k < n, else off: keep the classes with v_j >= the k-th largest logit counted with multiplicity
//                (ties at the k-th value all stay; fewer than k finite logits: all stay); Z_k = kept mass
//   top-p        0 < p < 1, else off, after top-k: class j stays iff the kept mass strictly above it is < p Z_k
//                (class 1 always stays, ties are never split); Z = kept mass after both cuts, kept = kept tokens
//   draw         h = mix(mix(seed + G) + G (c + 1)) mod 2^64, G = 0x9E3779B97F4A7C15, mix = splitmix64's finaliser;
//                u = ((h >> 40) + 0.5) 2^-24; token = the first one in canonical order whose cumulative mass exceeds u Z
//   side effects tok[r] = token, pos[r] += 1, kept[r] where asked for
//
// How: fp16 -> a monotone 16-bit key (sign flip; -0 joins +0).  The weight of a value is ONE number, fix(v) =
// trunc(expf((v - max) / T) 2^40) as a 64-bit integer, the same for every element of a class and wherever it is
// computed.  Passes over the row (it stays in L2; 300 KB at n = 152064):
//   1  maximum and its first index (argmax_step_kernel's scan)
//   2  coarse histogram by the key's high byte: count (u32) and mass (u64) per bucket, integer LDS atomics on 8 copies
//      (lane mod 8) that 256 threads add up afterwards
//   3  per search, a fine histogram (counts by the key's low byte) of the coarse bucket in which the threshold falls; the
//      mass of a fine bucket is count * fix(v).  The three searches are one routine, "the first key, descending, whose
//      inclusive prefix exceeds X": the k-th value (counts, X = k - 1), the p-cut (masses, X = ceil(p Z_k) - 1) and the
//      draw (masses, X = floor(u Z) = ((2 m + 1) Z) >> 25 in 128-bit integers, m = h >> 40).  A search that is off costs
//      nothing, one that lands in the coarse bucket of the search before it reuses that fine histogram: 1 to 3 passes.
//   4  rank r = (X - mass above the drawn class) / fix(v) inside the class: matches counted per round of 8192 elements
//      (integer LDS atomics), then a scan over the one round that holds the r-th match
// Prefix sums are integer scans (wave shuffles, then the wave totals in order).  No floating-point atomics and no
// floating-point sum at all; the only double is p * Z_k.  No scratch; LDS = kSmpLdsBytes = 26464 bytes, static:
// 8 x 256 (u32 + u64) coarse copies, 256 u32 fine, 128 u32 rounds, 16 (u32 + u64) wave totals, the 16 + 16 partials
// of the maximum, 32 bytes of results.
//
// Error bound delta: |prefix mass here / its float64 value on the same fp16 logits - 1| for any prefix of the canonical
// order (every such prefix holds class 1, so its mass is >= 1).  With a_i = (v_1 - v_i) / T >= 0, an element's weight
// e^-a_i is off by (a) the roundings of the difference and of the quotient, 2^-24 a_i each, carried through exp:
// relative 2^-23 a_i; (b) expf itself, at most 2 units of 2^-24 (OCML states 1 ulp); (c) the truncation to 2^-40 units,
// absolute 2^-40.  Summed over a prefix S with mass Z_S >= 1 and p_i = w_i / Z_S:
//   (a)  2^-23 sum p_i a_i = 2^-23 (H(p) - ln Z_S) <= 2^-23 ln |S| <= 2^-23 ln n     (a_i = -ln p_i - ln Z_S)
//   (b)  2^-23                                    (c)  n 2^-40 / Z_S <= n 2^-40
// Weights below 2^-40 (a_i > 27.7) count as 0 here: that is inside (c).  The thresholds are exact integers (the draw)
// or one double rounding (2^-52).  At n <= 2^20, the largest row the launch takes:
//   delta <= (13.9 + 1) 2^-23 + 2^-20 < 23 * 2^-23 < 2^-18.     kSmpDeltaLog2 = -18
// (n = 152064: 14.1 * 2^-23.)  The integer sums add nothing, so the bound does not grow with the order of anything.
// What a decision compares carries the error of two masses, the prefix C and u Z (or p Z_k), and still moves by at most
// delta Z, not 2 delta Z: (a) .. (c) bound the sum over ALL kept elements of |error of the element's weight| by delta Z
// (take S = the kept set), and C' - u Z' = (C - u Z) + (1 - u) (errors of the prefix) - u (errors of the rest): two
// disjoint sets of elements with factors in [0, 1].  So the kernel's token is one whose float64 interval comes within
// delta Z of u Z, and its p-cut differs from the float64 one only where a class boundary is within delta Z_k of p Z_k.
#pragma once
#include "launch.hip.h"
#include "nll_rows.hip.h"
#include "quip_device.hip.h"

namespace quip {
namespace {

constexpr int kSmpThreads = 1024;
constexpr int kSmpCopies = 8;                 // copies of the coarse histogram, by lane mod 8
constexpr int kSmpMaxRounds = 128;            // rounds of 8192 elements: n <= 2^20
constexpr int kSmpMaxN = kSmpMaxRounds * 8 * kSmpThreads;
typedef unsigned long long smp_u64;

// fp16 bits -> key, ascending with the value; 0 for what carries no mass (NaN, -inf).  +inf never gets here as a
// class: a row that holds one is greedy.  The smallest finite value, -65504 = 0xfbff, has key 0x0400.
__device__ __forceinline__ unsigned smp_key(unsigned h) {
  if ((h & 0x7fffu) > 0x7c00u || h == 0xfc00u) return 0;
  if (h == 0x8000u) h = 0;
  return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}

__device__ __forceinline__ float smp_value(unsigned key) {
  const unsigned short h = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return (float)__builtin_bit_cast(f16, h);
}

// the weight of every logit with this key, in units of 2^-40
__device__ __forceinline__ smp_u64 smp_fix(unsigned key, float m, float T) {
  return (smp_u64)(expf((smp_value(key) - m) / T) * 1099511627776.f);
}

__device__ __forceinline__ smp_u64 smp_mix(smp_u64 z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// inclusive prefix sum over threads 0 .. NT - 1 (NT = 256 or 1024) in thread order; every thread of the block calls it
template <int NT, class V>
__device__ __forceinline__ V smp_scan(V v, V* wsum, int tid) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V u = __shfl_up(v, o, 64);
    if ((tid & 63) >= o) v += u;
  }
  if (tid < NT && (tid & 63) == 63) wsum[tid >> 6] = v;
  __syncthreads();
  if (tid < NT)
    for (int w = 0; w < (tid >> 6); ++w) v += wsum[w];
  __syncthreads();
  return v;
}

struct SmpShared {
  smp_u64 cmass[kSmpCopies][256];
  unsigned ccnt[kSmpCopies][256];
  unsigned fcnt[256];
  unsigned rcnt[kSmpMaxRounds];
  smp_u64 wsum64[16];
  unsigned wsum32[16];
  float sv[16];
  int si[16];
  smp_u64 rmass[2];      // a search's answer: mass above the key | mass down to and including it
  unsigned rcount[2];    // the same in tokens
  int rkey;              // the key, -1: no prefix exceeds X
  int rpad;
};
constexpr int kSmpLdsBytes = 26464;
static_assert(sizeof(SmpShared) == kSmpLdsBytes, "sample_rows.hip.h: the LDS figure of the header comment");

__global__ __launch_bounds__(kSmpThreads) void sample_rows_kernel(const f16* __restrict__ logits, int n,
                                                                  const float* __restrict__ temperature,
                                                                  const int* __restrict__ top_k,
                                                                  const float* __restrict__ top_p,
                                                                  const int64_t* __restrict__ seed,
                                                                  int64_t* __restrict__ tok, int64_t* __restrict__ pos,
                                                                  int* __restrict__ kept) {
  __shared__ SmpShared S;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const f16* row = logits + (size_t)r * n;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int groups = (n + 7) >> 3;

  // pass 1: maximum and its first index (argmax_step_kernel's rule and start values)
  float best = -3.0e38f;
  int bi = 0x7fffffff;
  for (int g = tid; g < groups; g += kSmpThreads) nll_scan8(nll_load8(row, g, n, vec), g * 8, best, bi);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { S.sv[tid >> 6] = best; S.si[tid >> 6] = bi; }
  for (int i = tid; i < kSmpCopies * 256; i += kSmpThreads) { (&S.ccnt[0][0])[i] = 0; (&S.cmass[0][0])[i] = 0; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w)      // every thread, the same order (nll_rows_kernel)
    if (w != (tid >> 6) && (S.sv[w] > best || (S.sv[w] == best && S.si[w] < bi))) { best = S.sv[w]; bi = S.si[w]; }

  const float T = temperature[r];
  if (!(T > 0.f) || bi >= n || best == INFINITY) {          // greedy row (uniform over the block)
    if (tid == 0) {
      tok[r] = bi < n ? bi : 0;
      pos[r] += 1;
      if (kept) kept[r] = 1;
    }
    return;
  }
  const float m = best;

  // pass 2: coarse histogram
  {
    unsigned* cc = S.ccnt[tid & (kSmpCopies - 1)];
    smp_u64* cm = S.cmass[tid & (kSmpCopies - 1)];
    for (int g = tid; g < groups; g += kSmpThreads) {
      const uint4 q = nll_load8(row, g, n, vec);
      const unsigned* w = reinterpret_cast<const unsigned*>(&q);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned key = smp_key((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
        if (key) {
          atomicAdd(&cc[key >> 8], 1u);
          atomicAdd(&cm[key >> 8], smp_fix(key, m, T));
        }
      }
    }
  }
  __syncthreads();
  // thread d < 256 owns coarse bucket 255 - d: descending scans of counts and masses
  unsigned cown = 0, cinc;
  smp_u64 mown = 0, minc;
  if (tid < 256) {
#pragma unroll
    for (int c = 0; c < kSmpCopies; ++c) { cown += S.ccnt[c][255 - tid]; mown += S.cmass[c][255 - tid]; }
  }
  cinc = smp_scan<256>(cown, S.wsum32, tid);
  minc = smp_scan<256>(mown, S.wsum64, tid);
  if (tid == 255) { S.rcount[1] = cinc; S.rmass[1] = minc; }
  __syncthreads();
  const unsigned n_finite = S.rcount[1];
  const smp_u64 z_all = S.rmass[1];
  int loaded = -1;                  // the coarse bucket whose fine histogram S.fcnt holds

  // the first key, descending, whose inclusive prefix of masses (by_mass) or counts exceeds X -> S.rkey (-1: none),
  // S.rmass / S.rcount = what lies above it | down to and including it
  auto search = [&](bool by_mass, smp_u64 X) {
    __syncthreads();                // (the answer of the search before this one has been read)
    if (tid == 0) S.rkey = -1;
    __syncthreads();
    if (tid < 256) {
      const smp_u64 inc = by_mass ? minc : (smp_u64)cinc, own = by_mass ? mown : (smp_u64)cown;
      if (inc > X && inc - own <= X) { S.rkey = 255 - tid; S.rcount[0] = cinc - cown; S.rmass[0] = minc - mown; }
    }
    __syncthreads();
    const int B = S.rkey;
    if (B < 0) return;              // (uniform)
    const unsigned c_above = S.rcount[0];
    const smp_u64 m_above = S.rmass[0];
    if (B != loaded) {
      if (tid < 256) S.fcnt[tid] = 0;
      __syncthreads();
      for (int g = tid; g < groups; g += kSmpThreads) {
        const uint4 q = nll_load8(row, g, n, vec);
        const unsigned* w = reinterpret_cast<const unsigned*>(&q);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned key = smp_key((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
          if (key && (int)(key >> 8) == B) atomicAdd(&S.fcnt[key & 255u], 1u);
        }
      }
      loaded = B;
    }
    __syncthreads();                // (fcnt complete; rkey read by everyone)
    const unsigned key = ((unsigned)B << 8) | (unsigned)(255 - (tid & 255));
    const unsigned fc = tid < 256 ? S.fcnt[255 - tid] : 0u;
    const smp_u64 fm = (tid < 256 && fc && key) ? (smp_u64)fc * smp_fix(key, m, T) : 0ull;
    const unsigned fci = smp_scan<256>(fc, S.wsum32, tid) + c_above;
    const smp_u64 fmi = smp_scan<256>(fm, S.wsum64, tid) + m_above;
    if (tid == 0) S.rkey = -1;
    __syncthreads();
    if (tid < 256) {
      const smp_u64 inc = by_mass ? fmi : (smp_u64)fci, own = by_mass ? fm : (smp_u64)fc;
      if (inc > X && inc - own <= X) {
        S.rkey = (int)key;
        S.rcount[0] = fci - fc; S.rcount[1] = fci;
        S.rmass[0] = fmi - fm; S.rmass[1] = fmi;
      }
    }
    __syncthreads();
  };

  // top-k, then top-p: Z and the number of kept tokens
  smp_u64 Z = z_all;
  unsigned nkept = n_finite;
  const int k = top_k[r];
  if (k >= 1 && k < n && (unsigned)k < n_finite) {
    search(false, (smp_u64)(k - 1));
    if (S.rkey >= 0) { Z = S.rmass[1]; nkept = S.rcount[1]; }
  }
  const float p = top_p[r];
  if (p > 0.f && p < 1.f) {
    const double t = ceil((double)p * (double)Z);
    smp_u64 pI = (smp_u64)t;
    pI = pI < 1 ? 1 : (pI > Z ? Z : pI);
    search(true, pI - 1);
    if (S.rkey >= 0) { Z = S.rmass[1]; nkept = S.rcount[1]; }
  }

  // the draw
  const smp_u64 G = 0x9E3779B97F4A7C15ull;
  const smp_u64 h = smp_mix(smp_mix((smp_u64)seed[r] + G) + G * ((smp_u64)pos[r] + 1ull));
  const smp_u64 um = 2ull * (h >> 40) + 1ull;                                   // u = um 2^-25
  const smp_u64 X = (__umul64hi(um, Z) << 39) | ((um * Z) >> 25);               // floor(u Z) < Z
  search(true, X);
  const int kd = S.rkey;
  if (kd < 0) {                     // cannot happen (X < Z = a prefix's mass); the greedy token rather than a fault
    if (tid == 0) {
      tok[r] = bi;
      pos[r] += 1;
      if (kept) kept[r] = (int)nkept;
    }
    return;
  }
  const smp_u64 fixd = smp_fix((unsigned)kd, m, T);                              // > 0: the class's mass exceeds 0
  const unsigned cls = S.rcount[1] - S.rcount[0];
  unsigned rank = (unsigned)((X - S.rmass[0]) / (fixd ? fixd : 1ull));
  if (rank >= cls) rank = cls - 1;                                              // (cannot happen either)

  // pass 4: the rank-th index, ascending, among the logits of the drawn class
  if (tid < kSmpMaxRounds) S.rcnt[tid] = 0;
  __syncthreads();
  for (int g = tid; g < groups; g += kSmpThreads) {
    const uint4 q = nll_load8(row, g, n, vec);
    const unsigned* w = reinterpret_cast<const unsigned*>(&q);
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) c += smp_key((w[j >> 1] >> (16 * (j & 1))) & 0xffffu) == (unsigned)kd;
    if (c) atomicAdd(&S.rcnt[g >> 10], c);
  }
  __syncthreads();
  const unsigned rc = tid < kSmpMaxRounds ? S.rcnt[tid] : 0u;
  const unsigned rci = smp_scan<256>(rc, S.wsum32, tid);
  if (tid < kSmpMaxRounds && rci > rank && rci - rc <= rank) { S.rkey = tid; S.rcount[0] = rank - (rci - rc); }
  __syncthreads();
  const int g = S.rkey * kSmpThreads + tid;                 // this thread's group of the round that holds the match
  const unsigned in_round = S.rcount[0];
  unsigned mask = 0;
  if (g < groups) {
    const uint4 q = nll_load8(row, g, n, vec);
    const unsigned* w = reinterpret_cast<const unsigned*>(&q);
#pragma unroll
    for (int j = 0; j < 8; ++j) mask |= (unsigned)(smp_key((w[j >> 1] >> (16 * (j & 1))) & 0xffffu) == (unsigned)kd) << j;
  }
  const unsigned pc = __popc(mask);
  const unsigned pci = smp_scan<1024>(pc, S.wsum32, tid);
  if (pci > in_round && pci - pc <= in_round) {
    unsigned skip = in_round - (pci - pc);
    int j = 0;
    for (; j < 8; ++j)
      if ((mask >> j) & 1u) {
        if (skip == 0) break;
        --skip;
      }
    tok[r] = (int64_t)g * 8 + j;
    pos[r] += 1;
    if (kept) kept[r] = (int)nkept;
  }
}
}  // namespace

int sample_rows_launch(const void* logits, int rows, int n, const float* temperature, const int32_t* top_k,
                       const float* top_p, const int64_t* seed, int64_t* tok, int64_t* pos, int32_t* kept,
                       hipStream_t stream) {
  if (rows < 1 || n < 1 || n > kSmpMaxN) return QUIP_ERR_BAD_SHAPE;
  return launch<sample_rows_kernel>(dim3(rows), dim3(kSmpThreads), 0, stream, reinterpret_cast<const f16*>(logits), n,
                                    temperature, top_k, top_p, seed, tok, pos, kept);
}

}  // namespace quip
