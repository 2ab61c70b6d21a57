// LoRA adapters as a side branch of the quantised modules, one adapter index per row (punica / S-LoRA's batched shrink
// and expand).  Part of decode_glue.hip's translation unit.  Both launches are row-wise: a row's result is a function of
// that row's inputs, its adapter index and that adapter's weights -- not of the number of rows, the row's place or its
// neighbours -- and every order of additions is fixed.
//
// lora_shrink_rows_kernel<MODE>: t[row, r] = sum_k A[a, r, k] xin(row)[k], a = row_adapter[row]; x (rows, in) fp16,
// A (n_adapters, R, in) fp16, t (rows, R) fp32.  xin is the input the base module sees, in fp32 without an fp16 rounding,
// from the expressions of the input-side transform (had_device.hip.h):
//   MODE 0  x                                             (o_proj)
//   MODE 1  (x * rms_scale(1, sum x^2, in, eps)) * w      (q / k / v, gate / up: the RMSNorm of their Hadamard launch)
//   MODE 2  x * had::silu(gate)                           (down_proj)
// grid (rows, R / 8), 512 threads: the workgroup stages xin once in LDS as fp32 (in <= 28672: 112 KB), then wave w takes
// rank 8 blockIdx.y + w: lane l the 16-byte pieces l, l + 64, ... of A's row, fp32 FMA in increasing k, then the xor
// butterfly over the 64 lanes.  The sum of squares: thread t the pieces t, t + 512, ..., the same butterfly, the eight wave
// partials added in wave order.  A row without an adapter (index outside [0, n_adapters)) gets zeros; A is not read.
//
// lora_expand_rows_kernel: for up to three segments j (q / k / v, gate / up) in one launch
//   y_j[row, o] = fp16(fma(scale[a, j], sum_{r < R_j} float(B_j[a, o, r]) t[row, r0_j + r], float(y_j[row, o])))
// the sum by fp32 FMA in increasing r from 0.  grid (rows, sum_j ceil(out_j / 256)), 256 threads, one output per thread:
// its B row is R_j / 8 loads of 16 bytes, t is uniform over the workgroup.  A row without an adapter writes nothing.
#pragma once
#include "had_device.hip.h"
#include "launch.hip.h"
#include "quip_device.hip.h"

namespace quip {
namespace {

constexpr int kLoraWaves = 8;            // ranks per workgroup of the shrink launch
constexpr int kLoraLdsHead = 16;         // floats in front of the staged row: the wave partials of the sum of squares
constexpr int kLoraMaxIn = 28672;
constexpr int kLoraMaxRank = 192;

// every lane gets the sum of the 64: s += xor(s, 1), 2, 4, ..., 32
__device__ __forceinline__ float lora_wave_sum(float s) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s = had::fadd(s, __shfl_xor(s, o, 64));
  return s;
}

template <int MODE>
__global__ __launch_bounds__(64 * kLoraWaves) void lora_shrink_rows_kernel(
    const f16* __restrict__ x, const f16* __restrict__ A, const int* __restrict__ row_adapter, float* __restrict__ t, int in,
    int R, int n_adapters, const f16* __restrict__ aux, float eps) {
  extern __shared__ float lora_lds[];
  float* xs = lora_lds + kLoraLdsHead;
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = blockIdx.y * kLoraWaves + wave;      // (R is a multiple of 8: r < R)
  const int a = row_adapter[row];
  if (a < 0 || a >= n_adapters) {                    // (uniform over the workgroup)
    if (lane == 0) t[row * R + r] = 0.f;
    return;
  }
  const int pieces = in >> 3;
  const uint4* xr = reinterpret_cast<const uint4*>(x + row * in);
  float rs = 1.f;
  if constexpr (MODE == 1) {
    float ss = 0.f;
    for (int p = tid; p < pieces; p += 64 * kLoraWaves) {
      float v[8];
      had::unpack8(xr[p], v);
      had::sumsq8(v, ss);
    }
    ss = lora_wave_sum(ss);
    if (lane == 0) lora_lds[wave] = ss;
    __syncthreads();
    float S = lora_lds[0];
#pragma unroll
    for (int w = 1; w < kLoraWaves; ++w) S = had::fadd(S, lora_lds[w]);
    rs = had::rms_scale(1.f, S, in, eps);
  }
  for (int p = tid; p < pieces; p += 64 * kLoraWaves) {
    float v[8];
    had::unpack8(xr[p], v);
    if constexpr (MODE == 1) {
      float w[8];
      had::unpack8(reinterpret_cast<const uint4*>(aux)[p], w);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = had::fmul(had::fmul(v[i], rs), w[i]);
    }
    if constexpr (MODE == 2) {
      float g[8];
      had::unpack8(reinterpret_cast<const uint4*>(aux + row * in)[p], g);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = had::fmul(v[i], had::silu(g[i]));
    }
    float4* dst = reinterpret_cast<float4*>(xs + 8 * p);
    dst[0] = make_float4(v[0], v[1], v[2], v[3]);
    dst[1] = make_float4(v[4], v[5], v[6], v[7]);
  }
  __syncthreads();
  const uint4* Ar = reinterpret_cast<const uint4*>(A + ((size_t)a * R + r) * in);
  float acc = 0.f;
  for (int p = lane; p < pieces; p += 64) {
    float w[8];
    had::unpack8(Ar[p], w);
    const float4* src = reinterpret_cast<const float4*>(xs + 8 * p);
    const float4 x0 = src[0], x1 = src[1];
    acc = __builtin_fmaf(w[0], x0.x, acc);
    acc = __builtin_fmaf(w[1], x0.y, acc);
    acc = __builtin_fmaf(w[2], x0.z, acc);
    acc = __builtin_fmaf(w[3], x0.w, acc);
    acc = __builtin_fmaf(w[4], x1.x, acc);
    acc = __builtin_fmaf(w[5], x1.y, acc);
    acc = __builtin_fmaf(w[6], x1.z, acc);
    acc = __builtin_fmaf(w[7], x1.w, acc);
  }
  acc = lora_wave_sum(acc);
  if (lane == 0) t[row * R + r] = acc;
}

// (no arrays: a segment picked by blockIdx.y out of an array in the argument block would go through scratch)
struct LoraExpandArgs {
  f16 *y0, *y1, *y2;
  const f16 *b0, *b1, *b2;
  int out0, out1, out2;
  int R0, R1, R2;
  int r00, r01, r02;
  int tiles0, tiles1;       // workgroups of segments 0 and 1 along grid.y (segment 2 has the rest)
  const float* t;
  const float* scale;       // (n_adapters, 3)
  const int* row_adapter;
  int n_adapters, Rt;       // Rt: row length of t
};

__global__ __launch_bounds__(256) void lora_expand_rows_kernel(LoraExpandArgs a) {
  const size_t row = blockIdx.x;
  const int ad = a.row_adapter[row];
  if (ad < 0 || ad >= a.n_adapters) return;
  const int by = blockIdx.y;
  const int j = by < a.tiles0 ? 0 : (by < a.tiles0 + a.tiles1 ? 1 : 2);
  const int tile = by - (j == 0 ? 0 : (j == 1 ? a.tiles0 : a.tiles0 + a.tiles1));
  f16* y = j == 0 ? a.y0 : (j == 1 ? a.y1 : a.y2);
  const f16* B = j == 0 ? a.b0 : (j == 1 ? a.b1 : a.b2);
  const int out = j == 0 ? a.out0 : (j == 1 ? a.out1 : a.out2);
  const int R = j == 0 ? a.R0 : (j == 1 ? a.R1 : a.R2);
  const int r0 = j == 0 ? a.r00 : (j == 1 ? a.r01 : a.r02);
  const int o = tile * 256 + (int)threadIdx.x;
  if (o >= out) return;
  const uint4* Br = reinterpret_cast<const uint4*>(B + ((size_t)ad * out + o) * R);
  const float* tr = a.t + row * a.Rt + r0;
  float acc = 0.f;
  for (int r8 = 0; r8 < R; r8 += 8) {
    float b[8];
    had::unpack8(Br[r8 >> 3], b);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = __builtin_fmaf(b[i], tr[r8 + i], acc);
  }
  f16* yp = y + row * out + o;
  *yp = (f16)__builtin_fmaf(a.scale[ad * 3 + j], acc, (float)*yp);
}

}  // namespace

int lora_shrink_rows_launch(const void* x, const void* A, const int32_t* row_adapter, float* t, int64_t rows, int in, int R,
                            int n_adapters, int mode, const void* aux, float eps, hipStream_t stream) {
  if (rows < 1 || rows > 0x7fffffffll || n_adapters < 1 || in < 8 || in % 8 != 0 || R < 8 || R % 8 != 0 || mode < 0 || mode > 2)
    return QUIP_ERR_BAD_SHAPE;
  if (in > kLoraMaxIn || R > kLoraMaxRank) return QUIP_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)rows, R / kLoraWaves), block(64 * kLoraWaves);
  const int lds = (kLoraLdsHead + in) * (int)sizeof(float);
  const f16* xp = reinterpret_cast<const f16*>(x);
  const f16* Ap = reinterpret_cast<const f16*>(A);
  const f16* auxp = reinterpret_cast<const f16*>(aux);
  if (mode == 1) return launch<lora_shrink_rows_kernel<1>>(grid, block, lds, stream, xp, Ap, row_adapter, t, in, R, n_adapters, auxp, eps);
  if (mode == 2) return launch<lora_shrink_rows_kernel<2>>(grid, block, lds, stream, xp, Ap, row_adapter, t, in, R, n_adapters, auxp, eps);
  return launch<lora_shrink_rows_kernel<0>>(grid, block, lds, stream, xp, Ap, row_adapter, t, in, R, n_adapters, auxp, eps);
}

int lora_expand_rows_launch(const float* t, const int32_t* row_adapter, const float* scale, int64_t rows, int Rt, int n_adapters,
                            int segments, void* const* y, const void* const* B, const int32_t* out, const int32_t* R,
                            const int32_t* r0, hipStream_t stream) {
  if (rows < 1 || rows > 0x7fffffffll || n_adapters < 1 || segments < 1 || segments > 3 || Rt < 8 || Rt % 8 != 0)
    return QUIP_ERR_BAD_SHAPE;
  if (Rt > kLoraMaxRank) return QUIP_ERR_UNSUPPORTED;
  LoraExpandArgs a{};
  int tiles[3] = {0, 0, 0}, outs[3] = {0, 0, 0}, Rs[3] = {8, 8, 8}, r0s[3] = {0, 0, 0};
  const f16* Bs[3] = {nullptr, nullptr, nullptr};
  f16* ys[3] = {nullptr, nullptr, nullptr};
  for (int j = 0; j < segments; ++j) {
    if (out[j] < 0 || out[j] % 8 != 0 || R[j] < 8 || R[j] % 8 != 0 || r0[j] < 0 || r0[j] % 8 != 0 || r0[j] + R[j] > Rt)
      return QUIP_ERR_BAD_SHAPE;
    if (out[j] == 0) continue;                  // (a skipped segment: its pointers are not looked at)
    if (!y[j] || !B[j]) return QUIP_ERR_NULL_POINTER;
    if (!aligned16(B[j]) || (reinterpret_cast<uintptr_t>(y[j]) & 1)) return QUIP_ERR_MISALIGNED;
    outs[j] = out[j]; Rs[j] = R[j]; r0s[j] = r0[j];
    tiles[j] = (out[j] + 255) / 256;
    ys[j] = reinterpret_cast<f16*>(y[j]);
    Bs[j] = reinterpret_cast<const f16*>(B[j]);
  }
  const long long ny = (long long)tiles[0] + tiles[1] + tiles[2];
  if (ny == 0) return QUIP_OK;                  // every segment skipped: nothing to launch
  if (ny > 65535) return QUIP_ERR_BAD_SHAPE;
  a.y0 = ys[0]; a.y1 = ys[1]; a.y2 = ys[2];
  a.b0 = Bs[0]; a.b1 = Bs[1]; a.b2 = Bs[2];
  a.out0 = outs[0]; a.out1 = outs[1]; a.out2 = outs[2];
  a.R0 = Rs[0]; a.R1 = Rs[1]; a.R2 = Rs[2];
  a.r00 = r0s[0]; a.r01 = r0s[1]; a.r02 = r0s[2];
  a.tiles0 = tiles[0]; a.tiles1 = tiles[1];
  a.t = t; a.scale = scale; a.row_adapter = row_adapter; a.n_adapters = n_adapters; a.Rt = Rt;
  return launch<lora_expand_rows_kernel>(dim3((unsigned)rows, (unsigned)ny), dim3(256), 0, stream, a);
}

}  // namespace quip
