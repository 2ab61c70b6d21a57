// Prefill transform for rows of K x 512 and K x 1024 with any 2 <= K <= 48 (n <= 28672): the widths the batch kernels of
// hadamard.hip leave to the row-parallel latency kernel (13824 = 27 x 512, 18944 = 37 x 512, 17408 = 17 x 1024, ...).
// The arithmetic contract is had_transform_fused's on fp16 rows: input-side element work, the length-L Walsh-Hadamard
// transform of each of the K sub-rows, the K x K mix with had (or its transpose), scale, output-side element work, one
// rounding to fp16.
//
// One workgroup of 256 threads owns a token row at a time and walks over the rows on a persistent grid.  Per row:
//   (1) TRANSFORM FIRST, straight from the global loads.  The row is cut into units of 1024 consecutive elements; wave w
//       owns units w, w + 4, ...: two 16-byte pieces per lane, elements u 1024 + h 512 + 8 lane + [0, 8).  At L = 1024 a
//       unit is one sub-row (index bits 0..2 and 9 in registers, 3..8 across the lanes), at L = 512 two sub-rows side by
//       side (bits 0..2 in registers, 3..8 across the lanes) -- the same 16 registers, one register stage fewer.  The
//       butterflies are had_device's (packed fp32 in registers, DPP / swizzle between lanes) plus the two lane stages it
//       does not have: lane ^ 16 (ds_swizzle) and the half-wave exchange lane ^ 32 (ds_bpermute).
//   (2) the transformed values, times 2^-S (S = 4 / 5: about 1 / sqrt(L), so that they have the magnitude of the inputs
//       again and fit fp16), go to LDS as ONE 32-bit word each: fp16 hi | fp16 lo << 16, hi + lo = the value to 22 bits.
//       LDS map: [K][L + 8] words (the staged row, 16-byte aligned rows) | H as fp16 [48][48], zero outside (K, K).
//   (3) K-MIX on the matrix cores (v_mfma_f32_16x16x16_f16), two MFMAs per k step (hi, lo; products of two fp16 numbers
//       are exact in the fp32 accumulator).  A wave takes 128 consecutive columns; the MFMA's column lr of tile t is the
//       row's column 8 lr + t, so that after the eight tiles a lane holds eight CONSECUTIVE columns of each of its rows:
//       the epilogue scales, applies the output-side vectors and stores whole 16-byte pieces from the accumulators.
//       Its B operand is two 16-byte LDS reads per k (eight words = the eight tiles' hi and lo).
// This order needs one LDS write and one read per element and k-tile; mix first (had_tall_batch_kernel's order) would
// keep the output side at one MFMA per step but sends the fp32 mix result through LDS once more, into the transform's
// register layout, and its 112 KB.
// Order of the additions of an output element: the butterflies on index bits 0, 1, 2, (9 at L = 1024,) 3, ... 8, then
// k = 0, 16, 32: hi products then lo products of a step, inside a step the matrix core's order.  Nothing depends on the
// number of rows, on the row's place or on the grid.  No atomics, no scratch, plain vector stores.
// The next row's pieces (and the row's residual) are requested while the current row is in its mix; gfx9 counts loads
// and stores in one counter, so everything requested is waited for before the row's first store (landed()).
#include <hip/hip_runtime.h>

#include "had_device.hip.h"
#include "launch.hip.h"

namespace quip {
namespace {

struct MixArgs {
  const f16 *x, *had, *pre, *pre2, *gate, *post, *bias, *residual;
  f16* y;
  int in_features, out_features, n, K, transpose, rows;
  float scale;
};

constexpr int kHP = 48;   // H in LDS: 48 x 48 fp16 (three row tiles of 16)

__device__ __forceinline__ void mix_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// these requests have arrived, as far as the compiler's wait bookkeeping goes (see had_tall_batch_kernel)
template <int N>
__device__ __forceinline__ void landed(const u32x4 (&q)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" ::"v"(q[i]));
}
template <int N>
__device__ __forceinline__ void keep_packed(u32x4 (&q)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(q[i]));
}

// the lane stages had_device.hip.h does not have: partner lane ^ 16 (S = 4) and lane ^ 32 (S = 5)
template <int S>
__device__ __forceinline__ float lane_xor_far(float v, int lane) {
  const int i = __builtin_bit_cast(int, v);
  if constexpr (S == 4) return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(i, 0x401F));   // bit mode: xor 16
  else return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, i));
}
template <int S>
__device__ __forceinline__ void lane_stage_far(float v[16], int lane) {
#pragma clang fp contract(off)
  const float sg = ((lane >> S) & 1) ? -1.f : 1.f;
  const had::f32x2 sg2 = {sg, sg};
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const had::f32x2 own = {v[r], v[r + 1]}, par = {lane_xor_far<S>(v[r], lane), lane_xor_far<S>(v[r + 1], lane)};
    const had::f32x2 w = __builtin_elementwise_fma(own, sg2, par);   // (+-1) * own: exact product
    v[r] = w.x;
    v[r + 1] = w.y;
  }
}

// SIDE 0: no element-wise vectors, 1: input side (gate, pre, pre2), 2: output side (post, bias, residual)
template <int LOGL, int SIDE>
__global__ __launch_bounds__(256) void had_mix_batch_kernel(MixArgs a) {
#pragma clang fp contract(off)
  static_assert(LOGL == 9 || LOGL == 10, "L = 512 or 1024");
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));
  constexpr int L = 1 << LOGL, RS = L + 8;
  constexpr int MAXR = LOGL == 10 ? 7 : 6;       // units of 1024 elements per wave: n <= 28672 (K <= 48 at L = 512: 24576)
  constexpr int RTM = LOGL == 10 ? 2 : 3;        // row tiles of H: K <= 28 at L = 1024
  constexpr int CPW = L / 512;                   // 128-column chunks per wave
  constexpr int NE = CPW * RTM * 4;              // 16-byte pieces of an output-side vector per lane
  constexpr float kDown = LOGL == 10 ? 0.03125f : 0.0625f, kUp = LOGL == 10 ? 32.f : 16.f;
  extern __shared__ __attribute__((aligned(16))) uint32_t mix_lds[];
  const int K = a.K, n = a.n;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  uint32_t* const stage = mix_lds;
  f16* const hs = reinterpret_cast<f16*>(mix_lds + K * RS);

  u32x4 xq[MAXR * 2], gq[MAXR * 2], pq[MAXR * 2], p2q[MAXR * 2];   // x, gate (next row); pre, pre2 (all rows)
  u32x4 qpost[NE], qbias[NE], qres[NE];                            // post, bias (all rows); residual (this row)
  // first element of this lane's piece (r, h) of a row; pieces in [in_features, n) are requested at element 0 and count as zeros
  auto piece = [&](int r, int h) { return (wave + 4 * r) * 1024 + h * 512 + lane * 8; };
  auto fetch = [&](int row) {
    const char* xr = reinterpret_cast<const char*>(a.x + (int64_t)row * a.in_features);
    const char* gr = reinterpret_cast<const char*>(SIDE == 1 && a.gate ? a.gate + (int64_t)row * a.in_features : nullptr);
#pragma unroll
    for (int r = 0; r < MAXR; ++r)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int idx = piece(r, h);
        if (idx < n) {
          const uint32_t off = (uint32_t)(idx < a.in_features ? idx : 0) * 2u;
          xq[2 * r + h] = *reinterpret_cast<const u32x4*>(xr + off);
          if (SIDE == 1 && gr) gq[2 * r + h] = *reinterpret_cast<const u32x4*>(gr + off);
        }
      }
  };
  // element index of output piece (cc, rt, i) of this lane, or -1
  auto out_idx = [&](int cc, int rt, int i) {
    const int kp = rt * 16 + 4 * lq + i, idx = kp * L + (wave + 4 * cc) * 128 + 8 * lr;
    return (kp < K && idx < a.out_features) ? idx : -1;
  };

  int row = blockIdx.x;
  if (row < a.rows) fetch(row);
  if (SIDE == 1) {
#pragma unroll
    for (int r = 0; r < MAXR; ++r)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int idx = piece(r, h);
        if (idx < a.in_features) {
          if (a.pre) pq[2 * r + h] = *reinterpret_cast<const u32x4*>(a.pre + idx);
          if (a.pre2) p2q[2 * r + h] = *reinterpret_cast<const u32x4*>(a.pre2 + idx);
        }
      }
  }
  if (SIDE == 2) {
#pragma unroll
    for (int cc = 0; cc < CPW; ++cc)
#pragma unroll
      for (int rt = 0; rt < RTM; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int idx = out_idx(cc, rt, i), e = (cc * RTM + rt) * 4 + i;
          if (idx >= 0) {
            if (a.post) qpost[e] = *reinterpret_cast<const u32x4*>(a.post + idx);
            if (a.bias) qbias[e] = *reinterpret_cast<const u32x4*>(a.bias + idx);
          }
        }
  }
  // H as the MFMA's A operand, A[kq][k] at hs[kq * 48 + k], zero outside (K, K)
  for (int i = tid; i < kHP * kHP; i += 256) {
    const int kq = i / kHP, k = i - kq * kHP;
    hs[i] = (kq < K && k < K) ? (a.transpose ? a.had[k * K + kq] : a.had[kq * K + k]) : (f16)0.f;
  }
  // the loop starts with nothing pending
  landed(xq);
  if (SIDE == 1) { landed(gq); landed(pq); landed(p2q); }
  if (SIDE == 2) { landed(qpost); landed(qbias); }

  for (; row < a.rows; row += gridDim.x) {
    // (1) + (2): element-wise input work, transform, hi | lo image of the row in LDS
    if (SIDE == 1) { keep_packed(pq); keep_packed(p2q); }
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
      const int u = wave + 4 * r;
      if (u * 1024 < n) {
        float v[16];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          had::f32x2 o[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // F.pad zeros
          if (piece(r, h) < a.in_features) {   // (in_features <= n; a multiple of 8: a piece is all in or all out)
            had::unpack8p(xq[2 * r + h], o);
            if (SIDE == 1) {               // in the order of the single-row kernels: gate, pre, pre2
              if (a.gate) {
                had::f32x2 g[4];
                had::unpack8p(gq[2 * r + h], g);
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = o[i] * had::f32x2{had::silu(g[i].x), had::silu(g[i].y)};
              }
              if (a.pre) had::mul8p(o, pq[2 * r + h]);
              if (a.pre2) had::mul8p(o, p2q[2 * r + h]);
            }
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[8 * h + 2 * i] = o[i].x;
            v[8 * h + 2 * i + 1] = o[i].y;
          }
        }
        had::FhtPass<(LOGL == 10 ? 4 : 3), 0>::butterflies(v);
        had::lane_stage<0>(v, lane);
        had::lane_stage<1>(v, lane);
        had::lane_stage<2>(v, lane);
        had::lane_stage<3>(v, lane);
        lane_stage_far<4>(v, lane);
        lane_stage_far<5>(v, lane);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = LOGL == 10 ? u : 2 * u + h, j = (LOGL == 10 ? 512 * h : 0) + 8 * lane;
          if (k < K) {
            uint32_t w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const float t = v[8 * h + i] * kDown;
              const auto hi = __builtin_amdgcn_cvt_pkrtz(t, 0.f);
              w[i] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(t, t - (float)hi[0]));
            }
            uint32_t* dst = stage + k * RS + j;
            *reinterpret_cast<u32x4*>(dst) = u32x4{w[0], w[1], w[2], w[3]};
            *reinterpret_cast<u32x4*>(dst + 4) = u32x4{w[4], w[5], w[6], w[7]};
          }
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // (hoisted above the arithmetic, the requests would need a second set of registers)
    if (row + (int)gridDim.x < a.rows) fetch(row + gridDim.x);   // lands during the mix
    const f16* resr = SIDE == 2 && a.residual ? a.residual + (int64_t)row * a.out_features : nullptr;
    if (SIDE == 2 && resr) {
#pragma unroll
      for (int cc = 0; cc < CPW; ++cc)
#pragma unroll
        for (int rt = 0; rt < RTM; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int idx = out_idx(cc, rt, i);
            if (idx >= 0) qres[(cc * RTM + rt) * 4 + i] = *reinterpret_cast<const u32x4*>(resr + idx);
          }
    }
    mix_lds_barrier();
    // (3) K-mix and epilogue, 128 columns per wave and chunk
    f16* yr = a.y + (int64_t)row * a.out_features;
    const had::f32x2 sc = {a.scale * kUp, a.scale * kUp};   // (a power of two: the product rounds as v * scale does)
#pragma unroll
    for (int cc = 0; cc < CPW; ++cc) {
      const int cb = (wave + 4 * cc) * 128 + 8 * lr;
      f32x4 acc[RTM][8];
#pragma unroll
      for (int rt = 0; rt < RTM; ++rt)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < RTM; ++ks) {
        if (16 * ks < K) {
          f16x4v ah[RTM];
#pragma unroll
          for (int rt = 0; rt < RTM; ++rt)
            ah[rt] = *reinterpret_cast<const f16x4v*>(hs + (rt * 16 + lr) * kHP + 16 * ks + 4 * lq);
          u32x4 wq[4][2];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int k = min(16 * ks + 4 * lq + i, K - 1);   // (rows past K: any staged value, their column of H is zero)
            wq[i][0] = *reinterpret_cast<const u32x4*>(stage + k * RS + cb);
            wq[i][1] = *reinterpret_cast<const u32x4*>(stage + k * RS + cb + 4);
          }
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const uint32_t w0 = wq[0][t >> 2][t & 3], w1 = wq[1][t >> 2][t & 3], w2 = wq[2][t >> 2][t & 3],
                           w3 = wq[3][t >> 2][t & 3];
            const f16x4v bh = __builtin_bit_cast(f16x4v, uint2{(w0 & 0xffffu) | (w1 << 16), (w2 & 0xffffu) | (w3 << 16)});
            const f16x4v bl = __builtin_bit_cast(f16x4v, uint2{(w0 >> 16) | (w1 & 0xffff0000u), (w2 >> 16) | (w3 & 0xffff0000u)});
#pragma unroll
            for (int rt = 0; rt < RTM; ++rt) {
              if (rt * 16 < K) {
                acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah[rt], bh, acc[rt][t], 0, 0, 0);
                acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah[rt], bl, acc[rt][t], 0, 0, 0);
              }
            }
          }
        }
      }
      if (cc == 0) {
        // everything requested has had the mix to arrive; no load is waited for after the first store below
        landed(xq);
        if (SIDE == 1) landed(gq);
        if (SIDE == 2) { landed(qres); keep_packed(qpost); keep_packed(qbias); }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int rt = 0; rt < RTM; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int idx = out_idx(cc, rt, i), e = (cc * RTM + rt) * 4 + i;
          if (idx >= 0) {
            had::f32x2 o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = had::f32x2{acc[rt][2 * r][i], acc[rt][2 * r + 1][i]} * sc;
            if (SIDE == 2) {   // out_elem()'s order: scale, post, bias, residual, one rounding each
              if (a.post) had::mul8p(o, qpost[e]);
              if (a.bias) had::add8p(o, qbias[e]);
              if (resr) had::add8p(o, qres[e]);
            }
            *reinterpret_cast<uint4*>(yr + idx) = had::pack8p(o);
          }
        }
    }
    mix_lds_barrier();   // the image is rewritten for the next row
  }
}

template <auto Kern>
int mix_launch(const MixArgs& a, int lds, hipStream_t stream) {
  // persistent grid: as many workgroups as are resident at once (registers and LDS decide: 1 or 2 per CU), one row each
  // at a time.  Any number of rows goes out in one launch -- the rows are not a grid dimension, nothing to slice.
  if (ensure_dyn_lds(dyn_lds_state<Kern>(), reinterpret_cast<const void*>(Kern), lds) != QUIP_OK) return QUIP_ERR_LAUNCH;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kern, 256, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  const int64_t want = (int64_t)device_cu_count() * (per_cu < 4 ? per_cu : 4);
  const int gx = (int)(a.rows < want ? a.rows : want);
  return launch<Kern>(dim3(gx), dim3(256), lds, stream, a);
}

}  // namespace

int had_mix_batch_launch(const quip_had_problem* problem, int64_t rows, int n, int K, int transpose, hipStream_t stream) {
  const quip_had_problem& pr = *problem;
  if (!pr.x || !pr.out || !pr.had) return QUIP_ERR_NULL_POINTER;
  if (K < 1 || n < 1 || n % K != 0) return QUIP_ERR_BAD_SHAPE;
  const int L = n / K;
  if ((L & (L - 1)) != 0) return QUIP_ERR_BAD_SHAPE;
  if (pr.in_features < 1 || pr.out_features < 1 || pr.in_features > n || pr.out_features > n) return QUIP_ERR_BAD_SHAPE;
  // the kernel's scope
  if (K < 2 || K > 48 || (L != 512 && L != 1024) || n > 28672) return QUIP_ERR_UNSUPPORTED;
  if (rows < 32 || rows > 0x7fffffff) return QUIP_ERR_UNSUPPORTED;
  if (pr.rms_weight || pr.z) return QUIP_ERR_UNSUPPORTED;
  const bool in_side = pr.pre_scale || pr.pre_scale2 || pr.gate, out_side = pr.post_scale || pr.bias || pr.residual;
  if (in_side && out_side) return QUIP_ERR_UNSUPPORTED;
  if (pr.in_features % 8 != 0 || pr.out_features % 8 != 0) return QUIP_ERR_UNSUPPORTED;
  if (!aligned16(pr.x) || !aligned16(pr.out) || !aligned16(pr.pre_scale) || !aligned16(pr.pre_scale2) || !aligned16(pr.gate) ||
      !aligned16(pr.post_scale) || !aligned16(pr.bias) || !aligned16(pr.residual) || (reinterpret_cast<uintptr_t>(pr.had) & 1))
    return QUIP_ERR_UNSUPPORTED;
  MixArgs a{};
  a.x = reinterpret_cast<const f16*>(pr.x); a.had = reinterpret_cast<const f16*>(pr.had);
  a.pre = reinterpret_cast<const f16*>(pr.pre_scale); a.pre2 = reinterpret_cast<const f16*>(pr.pre_scale2);
  a.gate = reinterpret_cast<const f16*>(pr.gate); a.post = reinterpret_cast<const f16*>(pr.post_scale);
  a.bias = reinterpret_cast<const f16*>(pr.bias); a.residual = reinterpret_cast<const f16*>(pr.residual);
  a.y = reinterpret_cast<f16*>(pr.out);
  a.in_features = pr.in_features; a.out_features = pr.out_features; a.n = n; a.K = K; a.transpose = transpose;
  a.rows = (int)rows; a.scale = pr.scale;
  const int lds = K * (L + 8) * 4 + kHP * kHP * 2;
  const int side = in_side ? 1 : out_side ? 2 : 0;
  if (L == 512)
    return side == 0 ? mix_launch<had_mix_batch_kernel<9, 0>>(a, lds, stream)
         : side == 1 ? mix_launch<had_mix_batch_kernel<9, 1>>(a, lds, stream)
                     : mix_launch<had_mix_batch_kernel<9, 2>>(a, lds, stream);
  return side == 0 ? mix_launch<had_mix_batch_kernel<10, 0>>(a, lds, stream)
       : side == 1 ? mix_launch<had_mix_batch_kernel<10, 1>>(a, lds, stream)
                   : mix_launch<had_mix_batch_kernel<10, 2>>(a, lds, stream);
}

}  // namespace quip
