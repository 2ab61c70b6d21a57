// One LDLQ panel in one launch for the narrow codebooks: D4 (groups of 4 columns) and HI (groups of 1).
//
// The recursion of ldlq_panel_kernel (quantize.hip) over groups of b = kCodesz columns, per row over the c / b groups from
// the right:
//     t_k = B_k + sum_{j > k} (A_j - hat_j) M[j, k],   tgt_k = A_k + t_k P_k  (P == nullptr: A_k + t_k),   hat_k = Q(tgt_k)
// turned right-looking and kept in registers: with up to 128 groups of one column a left-looking step would be a workgroup
// barrier and a serial dot product per column.  kLanes lanes own a row (256 / kLanes rows per workgroup); group u lives on
// lane u % kLanes of its row in register slot u / kLanes, which holds the group's pending t (started from B) and its A.  The
// loop over k is fully unrolled (slots outer, lanes inner), so every register index is static.  One step: the owner lane
// forms tgt_k, the row's lanes take it (and A_k) by shuffles and round together, each lane then adds e_i M[k b + i, .] for
// e = A_k - hat_k to the slots it owns left of k -- its b consecutive floats of that row of M from LDS: the lanes of a row
// read one contiguous run, the rows of a wave the same addresses.  The running error never goes to LDS and the loop has no
// barrier.  A column's sum takes its terms in decreasing j, i ascending inside a group, whatever kLanes is, so a row's bits
// depend on that row alone.  The owner keeps hat_k and the code in the slot (A_k is dead by then) and stores after the loop.
// LDS (dynamic): M (c, c) | P (c / b, b, b) | for D4 the 256 entries (interleaved as e81b_slot does) and their squared norms.
// Rounding, with the first-maximum rule of torch.argmax over 2 x.g - |g|^2:
//   D4  dense arg max over the 256 entries: lane `sub` scans entries sub * (256 / kLanes) .. in increasing order (strict >),
//       products summed left to right without FMA, then the lanes agree on the higher score, then the lower index
//   HI  idx = clamp(ceil(t) + 7, 0, 15), hat = idx - 7.5: at an integer t the lower level wins, far targets saturate
// The shuffles are the swizzle / bpermute instructions themselves: inside 128 unrolled steps __shfl stays a call.
// This file has flags of its own in the build (EXTRA_FLAGS): no packed fp32 instructions, and no promotion of the slot arrays
// to 16-wide vectors, which costs the 8-lane HI instantiation 256 VGPRs and scratch (profiles/ldlq_small_panel_resources.txt).
#include <hip/hip_runtime.h>

#include "launch.hip.h"

namespace quip {

namespace {

constexpr int kSmallPanelMaxCols = 128;

// v of lane (lane ^ kOff), kOff < 32
template <int kOff>
__device__ __forceinline__ int swizzle_xor(int v) { return __builtin_amdgcn_ds_swizzle(v, (kOff << 10) | 0x1f); }

template <int kOff>
__device__ __forceinline__ void argmax_xor(float& best, int& key) {
  const float os = __int_as_float(swizzle_xor<kOff>(__float_as_int(best)));
  const int ok = swizzle_xor<kOff>(key);
  if (os > best || (os == best && ok < key)) { best = os; key = ok; }
}

// v of the lane whose byte address (4 * lane) is given
__device__ __forceinline__ float lane_read(float v, int addr) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
}

// entry e at slot (e % per) * kLanes + e / per, per = 256 / kLanes: the lanes of a row, which scan entries sub * per + i at
// the same i, read kLanes consecutive 16-byte pieces
template <int kLanes>
__device__ __forceinline__ int d4_slot(int e) { return (e % (256 / kLanes)) * kLanes + e / (256 / kLanes); }

// returns the index on every lane of the row; all of its kLanes lanes must call it
template <int kLanes>
__device__ __forceinline__ int d4_scan(const float (&x)[4], int sub, const float4* tb, const float* tn) {
#pragma clang fp contract(off)
  constexpr int kPer = 256 / kLanes;
  float best = -3.0e38f;
  int key = sub * kPer;
#pragma unroll 4
  for (int i = 0; i < kPer; ++i) {
    const int slot = i * kLanes + sub;
    const float4 g = tb[slot];
    float dot = x[0] * g.x;
    const float p1 = x[1] * g.y, p2 = x[2] * g.z, p3 = x[3] * g.w;
    dot = dot + p1;
    dot = dot + p2;
    dot = dot + p3;
    const float score = 2.f * dot - tn[slot];      // 2 * dot is exact: one rounding
    if (score > best) { best = score; key = sub * kPer + i; }
  }
  argmax_xor<1>(best, key);
  argmax_xor<2>(best, key);
  argmax_xor<4>(best, key);
  if constexpr (kLanes == 16) argmax_xor<8>(best, key);
  return key;
}

constexpr int ldlq_panel_small_lds_bytes(int c, int b) { return 4 * (c * c + c * b + (b == 4 ? 256 * 4 + 256 : 0)); }

template <int kCodesz, int kLanes>
__global__ __launch_bounds__(256, 2) void ldlq_panel_small_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                                 const float* __restrict__ M, const float* __restrict__ P,
                                                                 int64_t m, int c, const float* __restrict__ grid,
                                                                 float* __restrict__ hat, int64_t* __restrict__ idx) {
  static_assert((kCodesz == 4 || kCodesz == 1) && (kLanes == 8 || kLanes == 16), "D4 or HI, 8 or 16 lanes per row");
  constexpr int b = kCodesz;
  constexpr int kSlots = kSmallPanelMaxCols / (b * kLanes);
  extern __shared__ float small_lds[];
  float* Ms = small_lds;
  float* Ps = Ms + c * c;
  float4* tb = reinterpret_cast<float4*>(Ps + c * b);      // D4 only; c % 4 == 0 there, so 16-byte aligned
  float* tn = reinterpret_cast<float*>(tb + 256);
  const int groups = c / b;
  if ((c * c) % 4 == 0) {
    for (int i = threadIdx.x; i < c * c / 4; i += 256)
      reinterpret_cast<float4*>(Ms)[i] = reinterpret_cast<const float4*>(M)[i];
  } else {
    for (int i = threadIdx.x; i < c * c; i += 256) Ms[i] = M[i];
  }
  if (P != nullptr)
    for (int i = threadIdx.x; i < c * b; i += 256) Ps[i] = P[i];
  if constexpr (b == 4) {
    const float4 g = reinterpret_cast<const float4*>(grid)[threadIdx.x];
    const int slot = d4_slot<kLanes>(threadIdx.x);
    tb[slot] = g;
    tn[slot] = g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w;      // half-integers: exact in any order
  }
  __syncthreads();
  const int sub = threadIdx.x & (kLanes - 1), r = threadIdx.x / kLanes;
  const int row_lane0 = 4 * ((threadIdx.x & 63) - sub);      // byte address of the row's first lane for lane_read
  int64_t row = (int64_t)blockIdx.x * (256 / kLanes) + r;
  const bool valid = row < m;
  row = valid ? row : m - 1;      // rows past the end repeat the last row (they take part in the shuffles) and store nothing
  float t[kSlots][b], a[kSlots][b];
  int code[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int u = s * kLanes + sub;
    code[s] = 0;
#pragma unroll
    for (int i = 0; i < b; ++i) t[s][i] = a[s][i] = 0.f;
    if (u < groups) {
      if constexpr (b == 4) {
        const float4 av = *reinterpret_cast<const float4*>(A + row * c + u * 4);
        const float4 bv = *reinterpret_cast<const float4*>(B + row * c + u * 4);
        a[s][0] = av.x; a[s][1] = av.y; a[s][2] = av.z; a[s][3] = av.w;
        t[s][0] = bv.x; t[s][1] = bv.y; t[s][2] = bv.z; t[s][3] = bv.w;
      } else {
        a[s][0] = A[row * c + u];
        t[s][0] = B[row * c + u];
      }
    }
  }
#pragma unroll
  for (int s = kSlots - 1; s >= 0; --s) {
#pragma unroll
    for (int l = kLanes - 1; l >= 0; --l) {
      const int k = s * kLanes + l;
      if (k >= groups) continue;      // a short panel: uniform over the workgroup
      // every lane forms a target from its own slot s with group k's P (one broadcast read); only the owner's is taken
      float tg[b];
      if (P != nullptr) {
#pragma unroll
        for (int i = 0; i < b; ++i) {
          float acc = 0.f;
#pragma unroll
          for (int q = 0; q < b; ++q) acc = fmaf(t[s][q], Ps[(k * b + q) * b + i], acc);
          tg[i] = a[s][i] + acc;
        }
      } else {
#pragma unroll
        for (int i = 0; i < b; ++i) tg[i] = a[s][i] + t[s][i];
      }
      float x[b], ak[b], h[b];
#pragma unroll
      for (int i = 0; i < b; ++i) {
        x[i] = lane_read(tg[i], row_lane0 + 4 * l);
        ak[i] = lane_read(a[s][i], row_lane0 + 4 * l);
      }
      int cd;
      if constexpr (b == 4) {
        cd = d4_scan<kLanes>(x, sub, tb, tn);
        const float4 g = tb[d4_slot<kLanes>(cd)];
        h[0] = g.x; h[1] = g.y; h[2] = g.z; h[3] = g.w;
      } else {
        const float v = fminf(fmaxf(ceilf(x[0]) + 7.f, 0.f), 15.f);
        cd = (int)v;
        h[0] = v - 7.5f;
      }
      if (sub == l) {
        code[s] = cd;
#pragma unroll
        for (int i = 0; i < b; ++i) a[s][i] = h[i];
      }
      float e[b];
#pragma unroll
      for (int i = 0; i < b; ++i) e[i] = ak[i] - h[i];
#pragma unroll
      for (int s2 = 0; s2 <= s; ++s2) {
        if (s2 < s || sub < l) {      // groups left of k only: the triangle costs half, and column u b + i2 < k b <= c
          const float* mrow = Ms + (k * b) * c + (s2 * kLanes + sub) * b;
#pragma unroll
          for (int i = 0; i < b; ++i) {
            if constexpr (b == 4) {
              const float4 mv = *reinterpret_cast<const float4*>(mrow + i * c);
              t[s2][0] = fmaf(e[i], mv.x, t[s2][0]);
              t[s2][1] = fmaf(e[i], mv.y, t[s2][1]);
              t[s2][2] = fmaf(e[i], mv.z, t[s2][2]);
              t[s2][3] = fmaf(e[i], mv.w, t[s2][3]);
            } else {
              t[s2][0] = fmaf(e[i], mrow[i * c], t[s2][0]);
            }
          }
        }
      }
    }
  }
  if (!valid) return;
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int u = s * kLanes + sub;
    if (u < groups) {
      if constexpr (b == 4)
        *reinterpret_cast<float4*>(hat + row * c + u * 4) = make_float4(a[s][0], a[s][1], a[s][2], a[s][3]);
      else
        hat[row * c + u] = a[s][0];
      idx[row * groups + u] = (int64_t)code[s];
    }
  }
}

}  // namespace

// codesz 4: D4 with grid = its fp32 (256, 4) entries; codesz 1: HI (grid unused).  Lanes per row, from
// profiles/ldlq_small_bench.txt: a step is latency, not throughput, so 16 lanes (half the serial scan and half the updates per
// lane) win as long as their grid of m / 16 workgroups is resident at once -- two per CU is what the LDS admits (4096 rows on
// 256 CUs) -- and 8 lanes win once it is not and theirs still is (11008 rows).  QUIP_LDLQ_SMALL_LANES = 8 | 16 overrides the
// rule (tools/ldlq_bench.py measures both).
int ldlq_panel_small_launch(const void* A, const void* B, const void* M, const void* P, int64_t m, int c, const void* grid,
                            int codesz, void* hat, void* idx, hipStream_t stream) {
  if (m <= 0) return QUIP_OK;
  if ((codesz != 4 && codesz != 1) || c < codesz || c % codesz != 0 || c > kSmallPanelMaxCols) return QUIP_ERR_BAD_SHAPE;
  const int forced = env_int("QUIP_LDLQ_SMALL_LANES", 0);      // read per call: the tool alternates both in one process
  const int lanes = (forced == 8 || forced == 16) ? forced : (m + 15) / 16 <= 2 * (int64_t)device_cu_count() ? 16 : 8;
  const int rows = 256 / lanes;
  const int64_t blocks = (m + rows - 1) / rows;
  if (blocks > 0x7fffffff) return QUIP_ERR_BAD_SHAPE;
  auto go = [&](auto k) {
    return launch<decltype(k)::value>(dim3((unsigned)blocks), dim3(256), ldlq_panel_small_lds_bytes(c, codesz), stream,
                                      reinterpret_cast<const float*>(A), reinterpret_cast<const float*>(B),
                                      reinterpret_cast<const float*>(M), reinterpret_cast<const float*>(P), m, c,
                                      reinterpret_cast<const float*>(grid), reinterpret_cast<float*>(hat),
                                      reinterpret_cast<int64_t*>(idx));
  };
  if (codesz == 4)
    return lanes == 8 ? go(kernel_c<ldlq_panel_small_kernel<4, 8>>) : go(kernel_c<ldlq_panel_small_kernel<4, 16>>);
  return lanes == 8 ? go(kernel_c<ldlq_panel_small_kernel<1, 8>>) : go(kernel_c<ldlq_panel_small_kernel<1, 16>>);
}

}  // namespace quip
