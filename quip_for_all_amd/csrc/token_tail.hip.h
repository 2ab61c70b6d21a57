// The tail of a decoded token inside the persistent launch (decode_block.hip): final RMSNorm, lm_head, arg-max, next token.
//
// Behind the last block every one of the 256 resident workgroups holds the complete hidden state in registers (the residual
// stream `hreg`, strided layout: this thread's h[tid + 512 k], k < 8).  So the four launches that used to follow the blocks --
// RMSNorm, the dense fp16 lm_head product, the arg-max, and the embedding lookup of the NEXT step -- are work of the same
// launch:
//   norm     every workgroup normalises its own copy of h (sum of squares in fp64: it is 8 products per thread, and the
//            statistic is then exact against the one fp16 rounding of x) and keeps x = fp16(h * rsqrt(mean + eps) * w) as
//            4096 fp16 in LDS; every lane takes its fixed 64-element slice of x into 32 registers for the whole stream;
//   stream   workgroup w owns the rows [w q + min(w, r), +q (+1 for w < r)) of lm_head (vocab = 256 q + r), its eight waves
//            take them round robin; a row of 4096 fp16 is eight 16-byte nontemporal loads per lane and TWO rows per wave are
//            in flight (16 loads per lane, 128 KB per CU); products by v_dot2c_f32_f16 into four fp32 accumulators, one wave
//            reduction per row, the sum rounded to fp16 and stored (device scope);
//   arg-max  per wave, per workgroup, then ONE 8-byte granule {fp16 bits << 16 | local row, tag} per workgroup through the
//            launch's hand-off protocol (engine_sync.hip.h); workgroup 0 polls the 256 granules (bounded), reduces them and
//            stores the token and position + 1.  Rule of argmax_step_kernel (decode_glue.hip): argmax_better (quip_device.hip.h:
//            larger value, then lower index, NaN never wins), nothing found = token 0.
// A launch that gave up (ctl[1] != 0) answers like the separate launches do on an all-NaN hidden state: every logit NaN,
// token 0, position + 1.
#pragma once
#include <limits.h>

#include "engine_sync.hip.h"
#include "quip_device.hip.h"

namespace quip {
namespace tail {

struct Args {
  int64_t* tok = nullptr;          // device scalar: read at the top of the launch (by the caller), written here
  int64_t* pos = nullptr;          // device scalar: written pos + 1
  const f16* embed = nullptr;      // [vocab, 4096]
  const f16* norm_w = nullptr;     // final RMSNorm weight [4096], natural order
  const f16* lm_head = nullptr;    // [vocab, 4096] row-major, 16-byte aligned
  f16* logits = nullptr;           // [vocab]
  f16* xnorm = nullptr;            // optional debug output: the normalised hidden state [4096] (workgroup 0 writes it)
  int vocab = 0;                   // 256 <= vocab < 256 * 65535
};

constexpr int kHid = 4096, kWgs = 256, kWvs = 8, kThr = 512;
constexpr int kRowU4 = kHid / 8;                     // 16-byte pieces of a row
// The longest chain of fp32 roundings between the exact products and a logit: 8 dot2 steps per accumulator (two roundings
// each at worst: the instruction's internal precision is not specified), 2 additions that join the four accumulators, 6
// steps of the wave reduction.  (tests/test_gpu_token_tail.py derives its bound from this number.)
constexpr int kRoundingChain = 8 * 2 + 2 + 6;
constexpr int kLdsBytes = kHid * 2 + 256;            // x as fp16 | reduction slots
constexpr uint32_t kGiveUpCode = 0x9000u;

__device__ __forceinline__ void st_half_device(f16* p, uint16_t bits) {
  asm volatile("global_store_short %0, %1, off sc1" : : "v"(p), "v"((uint32_t)bits) : "memory");
}

// rows of workgroup w
__device__ __forceinline__ void row_range(int vocab, int w, int& row0, int& nrows) {
  const int q = vocab >> 8, r = vocab & 255;
  row0 = w * q + (w < r ? w : r);
  nrows = q + (w < r ? 1 : 0);
}

__device__ __forceinline__ float dot_row(const u32x4 (&W)[8], const u32x4 (&x)[8]) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a0 = __builtin_amdgcn_fdot2(as_f16x2(W[i].x), as_f16x2(x[i].x), a0, false);
    a1 = __builtin_amdgcn_fdot2(as_f16x2(W[i].y), as_f16x2(x[i].y), a1, false);
    a2 = __builtin_amdgcn_fdot2(as_f16x2(W[i].z), as_f16x2(x[i].z), a2, false);
    a3 = __builtin_amdgcn_fdot2(as_f16x2(W[i].w), as_f16x2(x[i].w), a3, false);
  }
  return (a0 + a1) + (a2 + a3);
}

// Every thread of every workgroup calls it (512 threads, 256 workgroups, all resident).  lds: kLdsBytes bytes, 16-byte
// aligned, nobody else's from here on.  gran: 256 granules of the workspace that no wait of this launch reads any more.
// tag: a tag no granule of `gran` can carry yet.  stamps: null, or 8 clock stamps of this workgroup.
__device__ __forceinline__ void run(const Args& t, const uint32_t (&hreg)[4], char* lds, uint32_t* ctl, uint64_t* gran,
                                    uint32_t tag, int w, float eps, long long pos64, uint64_t* stamps, bool stamps_rt) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#define TSTAMP(i) do { if (stamps && tid == 0) stamps[i] = stamps_rt ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime(); } while (0)
  TSTAMP(0);
  f16* xs = reinterpret_cast<f16*>(lds);
  double* redd = reinterpret_cast<double*>(lds + kHid * 2);              // [8] sums of squares
  float* redv = reinterpret_cast<float*>(lds + kHid * 2 + 64);           // [8] best values | [8] their rows
  int* redi = reinterpret_cast<int*>(lds + kHid * 2 + 96);

  // has a wait of this launch given up (or was the word set when it started)?  Whoever left a wait without its data has
  // seen the word before, and so has everybody who consumed what that workgroup published afterwards.
  uint32_t err;
  esync::ld4(err, ctl + 1);
  uint16_t wn[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) wn[k] = reinterpret_cast<const uint16_t*>(t.norm_w)[tid + 512 * k];
  esync::drain();
  esync::own(err);
  const bool failed = __builtin_amdgcn_readfirstlane((int)err) != 0;

  // ---- final RMSNorm ------------------------------------------------------------------------------------------------
  float h[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f16x2 hh = as_f16x2(hreg[j]);
    h[2 * j] = (float)hh.x;
    h[2 * j + 1] = (float)hh.y;
  }
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) ss = __builtin_fma((double)h[k], (double)h[k], ss);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o, 64);
  __builtin_amdgcn_s_barrier();                        // the area's earlier readers are done
  if (lane == 0) redd[wave] = ss;
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  double tot = 0.0;
#pragma unroll
  for (int i = 0; i < kWvs; ++i) tot += redd[i];
  const float rs = (float)(1.0 / __builtin_sqrt(tot * (1.0 / kHid) + (double)eps));
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const f16 xk = (f16)((h[k] * rs) * (float)__builtin_bit_cast(f16, wn[k]));
      xs[tid + 512 * k] = xk;
      if (t.xnorm && w == 0) t.xnorm[tid + 512 * k] = xk;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  u32x4 x[8];                                          // this lane's slice: elements [8 (64 i + lane), +8), i < 8
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = reinterpret_cast<const u32x4*>(lds)[64 * i + lane];
  TSTAMP(1);

  // ---- lm_head: this workgroup's rows, round robin over the waves, two rows per wave in flight ---------------------------
  int row0, nrows;
  row_range(t.vocab, w, row0, nrows);
  const u32x4* Wm = reinterpret_cast<const u32x4*>(t.lm_head) + (size_t)row0 * kRowU4 + lane;
  auto request = [&](int lr, u32x4 (&d)[8]) {
    const u32x4* p = Wm + (size_t)lr * kRowU4;
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = __builtin_nontemporal_load(p + 64 * i);
  };
  float best = -3.0e38f;
  int bi = INT_MAX;
  auto finish = [&](int lr, float s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    s = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, s)));
    const f16 hv = failed ? __builtin_bit_cast(f16, (uint16_t)0x7e00) : (f16)s;
    if (lane == 0) st_half_device(t.logits + row0 + lr, __builtin_bit_cast(uint16_t, hv));
    const float v = (float)hv;                         // the arg-max sees the logit as stored
    if (argmax_better(v, lr, best, bi)) { best = v; bi = lr; }
  };
  u32x4 A[8], Bw[8];
  if (wave < nrows) request(wave, A);
  if (wave + kWvs < nrows) request(wave + kWvs, Bw);
  for (int lr = wave; lr < nrows; lr += 2 * kWvs) {
    const float sa = dot_row(A, x);
    if (lr + 2 * kWvs < nrows) request(lr + 2 * kWvs, A);
    finish(lr, sa);
    if (lr + kWvs < nrows) {
      const float sb = dot_row(Bw, x);
      if (lr + 3 * kWvs < nrows) request(lr + 3 * kWvs, Bw);
      finish(lr + kWvs, sb);
    }
  }
  TSTAMP(2);

  // ---- arg-max: waves -> workgroup -> one granule --------------------------------------------------------------------
  esync::drain();                                      // this wave's logits are at the device scope before the granule says so
  if (lane == 0) { redv[wave] = best; redi[wave] = bi; }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (wave == 0) {
    best = redv[0]; bi = redi[0];
#pragma unroll
    for (int i = 1; i < kWvs; ++i)
      if (argmax_better(redv[i], redi[i], best, bi)) { best = redv[i]; bi = redi[i]; }
    const uint32_t word = ((uint32_t)__builtin_bit_cast(uint16_t, (f16)best) << 16) | (bi == INT_MAX ? 0xffffu : (uint32_t)bi);
    if (lane == 0) esync::st_granule(gran + w, word, tag);
  }
  TSTAMP(3);
  if (w != 0) return;

  // ---- workgroup 0: the 256 granules -> token, position -------------------------------------------------------------------
  asm volatile("s_barrier" ::: "memory");              // wave 0 has read the slots
  if (wave < 4) {
    esync::u32x2_t g;
    uint32_t spins = 0;
    for (;;) {
      esync::ld8(g, gran + tid);
      esync::drain();
      esync::own(g);
      if (esync::spin_step(g.y == tag, spins, ctl + 1, kGiveUpCode)) break;
    }
    int r0, nr;
    row_range(t.vocab, tid, r0, nr);
    const bool have = g.y == tag && (g.x & 0xffffu) != 0xffffu;
    float v = have ? (float)__builtin_bit_cast(f16, (uint16_t)(g.x >> 16)) : -3.0e38f;
    int idx = have ? r0 + (int)(g.x & 0xffffu) : INT_MAX;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (argmax_better(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
    if (lane == 0) { redv[wave] = v; redi[wave] = idx; }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  best = redv[0]; bi = redi[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (argmax_better(redv[i], redi[i], best, bi)) { best = redv[i]; bi = redi[i]; }
  uint32_t err2;
  esync::ld4(err2, ctl + 1);
  esync::drain();
  esync::own(err2);
  const bool failed2 = __builtin_amdgcn_readfirstlane((int)err2) != 0;
  if (failed2 && !failed) {
    // a wait gave up after this workgroup had looked: the other workgroups' logits are at the device scope (they drained
    // before their granule, or never wrote one) -- NaN over all of them
    for (int i = tid; i < t.vocab; i += kThr) st_half_device(t.logits + i, (uint16_t)0x7e00);
  }
  if (tid == 0) {
    *t.tok = (!failed2 && bi < t.vocab) ? (int64_t)bi : (int64_t)0;
    *t.pos = (int64_t)pos64 + 1;
  }
  TSTAMP(4);
#undef TSTAMP
}

}  // namespace tail
}  // namespace quip
