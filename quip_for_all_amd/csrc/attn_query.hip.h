// Single-query attention over a KV cache: the arithmetic that rope_attn_decode_kernel (decode_glue.hip) and the attention
// phases of the persistent launches (decode_block.hip, decode_block_gqa.hip) share bit for bit -- and, for rope8, the
// prompt-side launches (chunk_attn.hip.h), whose cache rows are the decode launch's.  This is the one place of it: the
// kernels keep their own walks over the cached rows (which rows a lane group visits, what is in flight) and call into this
// file for what they do to a key, a state or a pair of states.  A few call sites spell a primitive out instead, each with a
// remark at the site: update and both merges in rope_attn_decode_kernel, the merge of the head's parts in decode_block.hip
// (DESIGN.md 4.10 lists them, profiles/attn_primitives_refactor.txt has the reasons).
//
// A head vector of HD fp16 is spread over LPK = HD / 8 lanes, 16 bytes (8 dims) per lane; such a lane group walks its
// keys with an online-softmax state (m, l, acc[8]): running maximum, denominator, this lane's 8 unnormalised sums.
#pragma once
#include "had_device.hip.h"
#include "quip_device.hip.h"

namespace quip {
namespace attn {

__device__ __forceinline__ void unpack8h(const uint4& u, float o[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f16x2 h = as_f16x2(w[i]);
    o[2 * i] = (float)h.x;
    o[2 * i + 1] = (float)h.y;
  }
}

// ---- OCP e4m3fn cache rows (the fp8 paged launches, paged_attn.hip.h): a stored byte c means e4m3fn(c) * 2^e ----------
// 8 stored bytes -> the eight floats unpack8h gets from the fp16 row of the same values; sc = 2^e, the product is exact
__device__ __forceinline__ void unpack8f8(const uint2& u, float sc, float o[8]) {
  const uint32_t w[2] = {u.x, u.y};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    o[4 * i] = had::fmul(lo[0], sc);
    o[4 * i + 1] = had::fmul(lo[1], sc);
    o[4 * i + 2] = had::fmul(hi[0], sc);
    o[4 * i + 3] = had::fmul(hi[1], sc);
  }
}

// eight floats -> 8 bytes: x * 2^-e (isc, exact), finite values beyond +-448 and +-inf saturate to +-448, NaN stays NaN
// (compares, not fminf / fmaxf: those would swallow it), everything else rounds to nearest even, subnormals included.
// The saturation is done here: the conversion's own overflow behaviour is never reached.
__device__ __forceinline__ uint2 quant8f8(const float x[8], float isc) {
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    y[i] = had::fmul(x[i], isc);
    y[i] = y[i] > 448.f ? 448.f : y[i];
    y[i] = y[i] < -448.f ? -448.f : y[i];
  }
  uint2 u;
  u.x = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false), true);
  u.y = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false), true);
  return u;
}

// 2^e as a float, e in [-126, 127]
__device__ __forceinline__ float exp2i(int e) { return as_f32((uint32_t)(127 + e) << 23); }

// rotary embedding (HF half-rotation) of the 8 dims [d0, d0 + 8) of one head vector; result
// rounded to fp16 like the eager graph does
template <int HD>
__device__ __forceinline__ void rope8(const f16* vec, const float c8[8], const float s8[8], int d0, float o[8]) {
  float a[8], b[8];
  unpack8h(*reinterpret_cast<const uint4*>(vec + d0), a);
  const int dp = d0 < HD / 2 ? d0 + HD / 2 : d0 - HD / 2;
  unpack8h(*reinterpret_cast<const uint4*>(vec + dp), b);
  const float sgn = d0 < HD / 2 ? -1.f : 1.f;
#pragma unroll
  // x * cos + rot * sin with every operation rounded on its own, as the eager graph does (and so that the
  // instantiations of the kernels cannot contract the expression differently: an fma in one of them moved single
  // cache elements by one fp16 ulp)
  // (had::fmul / fadd: compiled with contraction switched off; __fmul_rn and friends are plain operators to hipcc)
  for (int i = 0; i < 8; ++i) o[i] = (float)(f16)had::fadd(had::fmul(a[i], c8[i]), had::fmul(sgn * b[i], s8[i]));
}

// ---- per-head RMSNorm of q / k in front of the rotation (Qwen3: q_norm / k_norm, a (HD,) weight each) ---------------------
// The one place of this arithmetic: qk_norm_rows_kernel (qk_norm.hip.h) and the kNorm instantiations of
// rope_attn_decode_kernel call these and nothing else for it, so the fused launch gives the bits of the stand-alone
// launch followed by the plain one.  Two fp16 roundings, HF's Qwen3RMSNorm.forward: normalised in fp32 and cast back,
// then the weight in fp16 (the product of two fp16 values is exact in fp32: one rounding).
//
// 1 / sqrt(mean(x^2) + eps) of a head vector; a8: this lane's 8 dims.  The lane's squares are added in index order from
// 0, the lane group's sums by had::sum16_xor; every lane of the group holds the result.  (v_sqrt_f32 and v_rcp_f32:
// one ulp each, the same instruction in every instantiation)
template <int HD>
__device__ __forceinline__ float inv_rms(const float (&a8)[8], float eps) {
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss = __builtin_fmaf(a8[i], a8[i], ss);
  const float S = had::sum16_xor<HD / 8>(ss);
  return __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(had::fadd(had::fmul(S, 1.f / HD), eps)));
}

// 8 dims of a head vector times r, rounded to fp16, times their 8 weights, rounded to fp16 (in place, as floats)
__device__ __forceinline__ void norm8(float (&a8)[8], float r, const f16* w8) {
  float w[8];
  unpack8h(*reinterpret_cast<const uint4*>(w8), w);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    // the fp32 product, THEN its conversion: left to the compiler, some of the products of an instantiation became
    // v_fma_mixlo_f16 (the exact product rounded once, to fp16) and the others v_mul_f32 + v_cvt_f16_f32 (rounded twice)
    // -- single elements of q moved by an fp16 ulp between the fused launch and the stand-alone one
    float p = had::fmul(a8[i], r);
    asm("" : "+v"(p));
    a8[i] = (float)(f16)had::fmul((float)(f16)p, w[i]);
  }
}

// rope8 of the NORMALISED head vector: the 8 dims at d0 and the 8 partner dims are normalised here, with the one r of
// the head (the lanes of the group hold the whole head: all of them call this together)
template <int HD>
__device__ __forceinline__ void rope8_norm(const f16* vec, const f16* w, float eps, const float c8[8], const float s8[8],
                                           int d0, float o[8]) {
  float a[8], b[8];
  unpack8h(*reinterpret_cast<const uint4*>(vec + d0), a);
  const int dp = d0 < HD / 2 ? d0 + HD / 2 : d0 - HD / 2;
  unpack8h(*reinterpret_cast<const uint4*>(vec + dp), b);
  const float r = inv_rms<HD>(a, eps);
  norm8(a, r, w + d0);
  norm8(b, r, w + dp);
  const float sgn = d0 < HD / 2 ? -1.f : 1.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (float)(f16)had::fadd(had::fmul(a[i], c8[i]), had::fmul(sgn * b[i], s8[i]));   // (rope8's expression)
}

// one key against q: this lane's 8 products, then the lane group's sum on DPP moves (had::sum16_xor: the additions of
// `s += __shfl_xor(s, o)`, o = 1, 2, 4, 8) -- every lane of the group holds the score
template <int LPK>
__device__ __forceinline__ float score(const float (&q8)[8], const float (&k8)[8]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s = __builtin_fmaf(q8[i], k8[i], s);
  return had::sum16_xor<LPK>(s);
}

// online-softmax step of one lane group's state with a key's score s and this lane's 8 values of its v row
// (spelled out: left to the compiler, the instantiations of a kernel contract a * c + p * v differently -- one element in
//  8192 moved by an ulp between the grouped-query prologue and the plain kernel)
__device__ __forceinline__ void update(float& m, float& l, float (&acc)[8], float s, const float (&v8)[8]) {
  const float mn = fmaxf(m, s);
  const float c = __expf(m - mn), p = __expf(s - mn);
  l = __builtin_fmaf(l, c, p);
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(acc[i], c, had::fmul(p, v8[i]));
  m = mn;
}

// Two lane groups of a wave merge their states in registers.  swap(x) hands every lane both partners' copies of x as
// {[0], [1]} -- v_permlane16_swap / 32_swap of a value with ITSELF: (even row, odd row) / (lower half, upper half) -- so
// both sides compute the same merged state and nobody selects.
template <class Swap>
__device__ __forceinline__ void merge2(float& m, float& l, float (&acc)[8], Swap swap) {
  const auto tm = swap(as_u32(m)), tl = swap(as_u32(l));
  const float mA = as_f32((uint32_t)tm[0]), mB = as_f32((uint32_t)tm[1]);
  const float M = fmaxf(mA, mB);
  const float wA = mA == -INFINITY ? 0.f : __expf(mA - M), wB = mB == -INFINITY ? 0.f : __expf(mB - M);
  l = __builtin_fmaf(as_f32((uint32_t)tl[1]), wB, had::fmul(as_f32((uint32_t)tl[0]), wA));
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const auto ta = swap(as_u32(acc[i]));
    acc[i] = __builtin_fmaf(as_f32((uint32_t)ta[1]), wB, had::fmul(as_f32((uint32_t)ta[0]), wA));
  }
  m = M;
}

// Weighted merge of N states (m_i, l_i, o_i), i in order, for ONE output dimension: the states of a workgroup's lane
// groups or waves out of LDS, the partial states of a head's workgroups out of the workspace.  State i: m[i * ml_stride],
// l[i * ml_stride], o[i * o_stride] (o: already moved to the caller's dimension).  (M, L, O) come in as (-inf, 0, 0).
// A state that saw no key (m = -inf) has weight 0.
template <int N>
__device__ __forceinline__ void merge_states(const float* m, const float* l, int ml_stride, const float* o, int o_stride,
                                             float& M, float& L, float& O) {
  for (int i = 0; i < N; ++i) M = fmaxf(M, m[i * ml_stride]);
  for (int i = 0; i < N; ++i) {
    const float mi = m[i * ml_stride];
    const float w = mi == -INFINITY ? 0.f : __expf(mi - M);
    L = __builtin_fmaf(l[i * ml_stride], w, L);
    O = __builtin_fmaf(o[i * o_stride], w, O);
  }
}

// ---- the cached rows of a head in the persistent launches (decode_block.hip, decode_block_gqa.hip) ------------------------
// A workgroup is part `part` of the `nparts` that share a head: it owns the positions part + nparts i below pos, i its
// local index.  Lane group g of NG takes the local indices g + NG j; a ROUND is U of them, i0 + u NG, u < U, their 16-byte
// pieces of the K and V rows in (kr, vr).  The kernels keep two rounds in flight and request a round two rounds ahead of
// its use; that loop, and the new row behind it, are theirs.
// Both structs hold references to the kernel's own variables and nothing else -- what its lambdas used to capture.
template <int HD, int U, int NG>
struct CachedRows {
  const f16* const& kc;      // the KV head's rows, [max_len, HD]
  const f16* const& vc;
  const int& part;
  const int& nparts;
  const int& pos;
  const int& d0;             // this lane's 8 dims
  __device__ __forceinline__ int position(int i) const { return part + nparts * i; }      // of local index i
  // request the round at local index i0 (a row at or past pos: row 0, never used).  Also called on its own, long before
  // q exists.
  __device__ __forceinline__ void load_round(uint4 (&kr)[U], uint4 (&vr)[U], int i0) const {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = position(i0 + u * NG);
      const int tc = t < pos ? t : 0;
      kr[u] = *reinterpret_cast<const uint4*>(kc + (size_t)tc * HD + d0);
      vr[u] = *reinterpret_cast<const uint4*>(vc + (size_t)tc * HD + d0);
    }
  }
};

// One round against q: all of its scores first (independent chains), then the updates of the group's state in key order
// -- the same operations on the same operands as key after key.
template <int HD, int U, int NG>
struct Round {
  const CachedRows<HD, U, NG>& rows;
  const float (&q8)[8];
  float& m;
  float& l;
  float (&acc)[8];
  __device__ __forceinline__ void operator()(const uint4 (&kr)[U], const uint4 (&vr)[U], int i0) const {
    float k8[U][8], v8[U][8], sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      unpack8h(kr[u], k8[u]);
      unpack8h(vr[u], v8[u]);
      sc[u] = score<HD / 8>(q8, k8[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (rows.position(i0 + u * NG) < rows.pos) update(m, l, acc, sc[u], v8[u]);
  }
};

}  // namespace attn
}  // namespace quip
