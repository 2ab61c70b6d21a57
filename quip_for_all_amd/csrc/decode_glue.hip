// bs=1 decode glue between the QuantLinear calls of one transformer block: rotary embedding of
// q / k, KV-cache append and single-query attention over the static cache, in one launch.
// This is the part of the reference's metric driver (example_generate.py:9-59: HF StaticCache +
// LlamaAttention under torch.compile) that sits between q/k/v_proj and o_proj; it is not part of
// quip_cuda.  Fused here because on MI355X every dependent launch of a decode step costs
// microseconds while the math is nothing.
//
// One workgroup per query head, 256 threads.  A key is handled by HD/8 lanes (16 bytes of the
// fp16 head vector per lane); the 256/(HD/8) lane groups stride over the cached positions with
// their own online-softmax state and are merged through LDS at the end (flash-decoding inside
// a workgroup).  The new k / v row is used from registers (and appended to the cache by the
// first query head of its KV group), so no other workgroup has to see the cache write.
// Contexts of a few thousand tokens are fine; beyond that a split over workgroups would pay.
//
// ZIN variant (round 2): the launch takes the RAW GEMV outputs of q / k / v_proj and runs their output-side
// Hadamard transform (SV (.) H z / sqrt(n), qlinear.py:106-114 with K = 1) in its own prologue -- three groups of 256
// threads transform q, k and v side by side with the functions of had_device.hip.h (the same bits as the separate
// transform launch it replaces), the 8 threads that own this head's 128 values leave them in LDS, and the
// attention proper continues on the first 256 threads.  Every head repeats the three 4096-point transforms
// (~0.5 us on otherwise idle CUs) instead of one more dependent launch per block (~5 us).
//
// Batched variant (SEQ): B independent sequences in one launch, sequence b = blockIdx.z with its own position pos[b],
// its own cache slice [b] (the bs=1 layout), its own partial states and arrival counters.  Per sequence the code path
// is the bs=1 kernel's (same lane groups, key order, split rule and merge), so every sequence's output and cache rows
// are bit identical to a bs=1 launch on that sequence alone.
#include <type_traits>

#include "attn_query.hip.h"
#include "had_device.hip.h"
#include "quip_device.hip.h"
#include "launch.hip.h"

namespace quip {
namespace {

struct AttnZ {
  const f16* z[3];      // raw GEMV outputs of q / k / v_proj, [n] each
  const f16* post[3];   // SV of the three modules, [n]
  float scale[3];       // 1 / sqrt(width)
  int n, logL;          // multi-head attention: common width (heads * HD == kv_heads * HD == n), a power of two <= 4096
                        // grouped queries (LQ / LKV instantiations): the width of q; k and v are 2^LKV wide
};

struct AttnArgs {
  const f16* q;        // [heads, HD]            (batched: [B, heads, HD])
  const f16* k;        // [kv_heads, HD]  (pre-rope; batched: [B, kv_heads, HD])
  const f16* v;        // [kv_heads, HD]
  const float* cos;    // [max_len, HD]
  const float* sin;    // [max_len, HD]
  const int64_t* pos;  // device scalar: index of the current token (batched: [B], one per sequence)
  f16* kcache;         // [kv_heads, max_len, HD]  (batched: [B, kv_heads, max_len, HD])
  f16* vcache;
  f16* out;            // [heads, HD]            (batched: [B, heads, HD])
  int heads, kv_heads, max_len;
  float scale;
  float* ws;           // split mode: partial (acc[HD], m, l) per (head, split); null: one workgroup per head
  unsigned* counters;  // split mode: arrivals per head (zero between launches)  (batched: per (sequence, head))
  int window;          // sliding-window attention (Mistral: config.sliding_window): positions (pos - window, pos]; <= 0: [0, pos]
  static constexpr bool kPaged = false;
  static constexpr bool kFp8 = false;
  static constexpr bool kStart = false;
  static constexpr bool kNorm = false;
};

// The batched launch on sequences that do not begin at cache row 0 (a left-padded batch): sequence b's tokens live in
// cache rows [start[b], pos[b]], row t has rotary position t - start[b].  Rows below start[b] are never read.
struct StartAttnArgs : AttnArgs {
  const int64_t* start;   // [B] device int64: first cache row of every sequence
  static constexpr bool kStart = true;
};

// The batched launch on a PAGED cache (paged_attn.hip.h): kcache / vcache are page pools, a row is found through the
// block table.  max_len stays the row count of cos / sin and the bound of the range rule.
constexpr int kPage = 64;             // positions per page == kChunkTile (chunk_attn.hip.h)
struct PagedAttnArgs : AttnArgs {
  const int32_t* table;   // [B, max_pages]: page of positions [64 j, 64 j + 64) of sequence b, -1: none
  int n_pages, max_pages; // kcache / vcache: [n_pages, kv_heads, kPage, HD]
  static constexpr bool kPaged = true;
};
// The same on pools of OCP e4m3fn bytes (paged_attn.hip.h): kcache / vcache point at one byte per element, a stored
// byte c of the K pool means e4m3fn(c) * 2^k_exp, of the V pool e4m3fn(c) * 2^v_exp.
struct PagedAttnArgsF8 : PagedAttnArgs {
  int k_exp, v_exp;       // in [-8, 7] (the launcher checks): every code times 2^e is an exact fp16 value
  static constexpr bool kFp8 = true;
};

// Any of the argument types with a per-head RMSNorm of q and of the new k row in front of the rotation (Qwen3's q_norm /
// k_norm; attn_query.hip.h: rope8_norm): the bits of qk_norm_rows_kernel (qk_norm.hip.h) on q and k followed by the launch
// on Base.  An argument TYPE, not one more template parameter: the instantiations on the plain types keep their names.
template <class Base>
struct QkNormArgs : Base {
  const f16* qw;          // [HD] weight of q's norm
  const f16* kw;          // [HD] weight of k's norm
  float eps;
  static constexpr bool kNorm = true;
};

constexpr int kSplits = 8;  // workgroups per head for long contexts (grid.y)
constexpr int kSplitFromPos = 256;    // shorter contexts: split 0 does everything, no workspace traffic

// barriers inside fht16_fixed<LOGL, false> (had_device.hip.h): two around the lane stages, two per pass through LDS
__host__ __device__ constexpr int fht16_barriers(int logl) { return logl <= 8 ? 2 : 2 + 2 * ((logl + 3) / 4 - 2); }

// ZIN with LQ == 0: q, k, v of one common width on 3 x 256 threads (run-time length).  LQ > 0 (grouped queries): q of
// width 2^LQ on the first 2^LQ / 16 threads, k and v of width 2^LKV on the next 2 x 2^LKV / 16 (whole waves each).
// SEQ: the batched launch -- blockIdx.z selects the sequence; the pointers move to its tensors before anything is read.
// Args: AttnArgs, or PagedAttnArgs (SEQ only) -- the same walk, split rule, window rule and merge with every cache row
// addressed through the sequence's block-table row, which the workgroup validates and brings into LDS first.
// PagedAttnArgsF8: the paged walk on byte pools -- a lane loads 8 bytes per key instead of 16 and converts them to the
// eight floats the fp16 kernel unpacks (exact), and the new row is replaced by dequant(quant(.)) before it is used at
// t == pos, so what is scored now is what a later launch finds in the cache.
// StartAttnArgs (SEQ only): the contiguous walk from max(start[b], the window's first key) with q and the new k rotated
// by row pos - start[b] of cos / sin; start[b] outside [0, pos] joins the range rule.  All zeros: the AttnArgs launch's bits.
template <int HD, bool ZIN, int LQ = 0, int LKV = 0, bool SEQ = false, class Args = AttnArgs>
__global__ __launch_bounds__(!ZIN ? 256 : (LQ == 0 ? 768 : (1 << LQ) / 16 + 2 * ((1 << LKV) / 16)))
void rope_attn_decode_kernel(Args a, AttnZ zz) {
  constexpr bool PAGED = Args::kPaged;
  constexpr bool FP8 = Args::kFp8;
  constexpr bool START = Args::kStart;
  constexpr bool NORM = Args::kNorm;
  constexpr int LPK = HD / 8;        // lanes per key
  constexpr int NG = 256 / LPK;      // key groups per workgroup
  constexpr int U = 4;               // keys in flight per group
  static_assert(!(SEQ && ZIN), "the raw-GEMV-input variants are bs=1 only");
  static_assert(!PAGED || SEQ, "the paged cache belongs to the batched launch");
  static_assert(!FP8 || PAGED, "the fp8 cache is a paged cache");
  static_assert(!START || (SEQ && !PAGED), "a first row per sequence belongs to the contiguous batched launch");
  static_assert(!NORM || !ZIN, "the raw-GEMV-input variants have no q / k norm");
  __shared__ float s_m[NG], s_l[NG];
  __shared__ float s_acc[NG][HD + 4];
  const int tid = threadIdx.x, h = blockIdx.x;
  if constexpr (SEQ) {
    const size_t b = blockIdx.z;
    a.q += b * a.heads * HD;
    a.k += b * a.kv_heads * HD;
    a.v += b * a.kv_heads * HD;
    a.pos += b;
    if constexpr (START) a.start += b;
    if constexpr (PAGED) {
      a.table += b * a.max_pages;
    } else {
      a.kcache += b * a.kv_heads * (size_t)a.max_len * HD;
      a.vcache += b * a.kv_heads * (size_t)a.max_len * HD;
    }
    a.out += b * a.heads * HD;
    if (a.ws) {
      a.ws += b * a.heads * kSplits * (HD + 4);
      a.counters += b * a.heads;
    }
  }
  const int gl = tid % LPK, grp = tid / LPK, d0 = gl * 8;
  const int group = a.heads / a.kv_heads, kvh = h / group;
  // ZIN: the transform inputs do not depend on the position: requested before it is read
  constexpr bool GQ = LQ > 0;
  constexpr int TQ = GQ ? (1 << LQ) / 16 : 256, TKV = GQ ? (1 << LKV) / 16 : 256;
  static_assert(!GQ || (TQ >= 256 && TKV % 64 == 0), "the attention runs on the first 256 threads; k / v on whole waves");
  const int g3 = GQ ? (tid < TQ ? 0 : (tid < TQ + TKV ? 1 : 2)) : tid >> 8;
  const int tt = GQ ? tid - (g3 == 0 ? 0 : (g3 == 1 ? TQ : TQ + TKV)) : tid & 255, e0 = tt * 16;
  const bool zact = ZIN && (GQ || e0 < zz.n);
  uint4 zraw[2] = {}, praw[2] = {};
  if constexpr (ZIN) {
    if (zact) {
      zraw[0] = *reinterpret_cast<const uint4*>(zz.z[g3] + e0);
      zraw[1] = *reinterpret_cast<const uint4*>(zz.z[g3] + e0 + 8);
      praw[0] = *reinterpret_cast<const uint4*>(zz.post[g3] + e0);
      praw[1] = *reinterpret_cast<const uint4*>(zz.post[g3] + e0 + 8);
    }
  }
  const long long pos64 = *a.pos;
  // A position outside the cache (one step past max_len, a corrupted counter) must not index cos / sin or the
  // cache: nothing is appended, the head's output becomes NaN (visible downstream) and every workgroup of the
  // launch leaves before touching the split workspace.
  if (pos64 < 0 || pos64 >= (long long)a.max_len) {
    if (blockIdx.y == 0 && tid < HD) a.out[(size_t)h * HD + tid] = __builtin_bit_cast(f16, (unsigned short)0x7e00);
    return;
  }
  const int pos = (int)pos64;
  int start = 0;
  if constexpr (START) {
    // the range rule's two further conditions: the sequence begins inside [0, pos]
    const long long start64 = *a.start;
    if (start64 < 0 || start64 > pos64) {
      if (blockIdx.y == 0 && tid < HD) a.out[(size_t)h * HD + tid] = __builtin_bit_cast(f16, (unsigned short)0x7e00);
      return;
    }
    start = (int)start64;
  }
  // split mode (long context, workspace given): workgroup (h, s) takes positions [t_lo, t_hi); the last
  // workgroup of a head to arrive merges the partial softmax states (flash-decoding across CUs)
  const bool split = a.ws != nullptr && pos >= kSplitFromPos;
  const int sidx = blockIdx.y;
  if (!split && sidx > 0) return;
  // sliding window: the walk starts at `first` instead of 0 (the cache stays linear: rows [0, pos] all exist)
  // (START: never below the sequence's first row)
  const int first = START ? max(start, a.window > 0 ? pos + 1 - a.window : 0)
                          : (a.window > 0 ? max(0, pos + 1 - a.window) : 0);
  const int chunk = split ? (pos - first + kSplits) / kSplits : pos + 1 - first;      // ceil((pos + 1 - first) / kSplits)
  const int t_lo = first + (split ? sidx * chunk : 0);
  const int t_hi = split ? min(pos + 1, t_lo + chunk) : pos + 1;       // exclusive (a split past the end walks nothing: m = -inf)
  if constexpr (PAGED) {
    // Table validity, part of the range rule: an entry of pages first >> 6 .. pos >> 6 outside [0, n_pages) -> no
    // append, NaN heads, no workspace traffic.  Every wave scans the whole range itself (one entry per lane and
    // round), so all waves of all workgroups of the sequence reach the same verdict without an exchange; wave 0
    // leaves the row in LDS on the way, and the key loop's addresses come from there.  Pages below the window's first
    // page are not looked at.
    extern __shared__ int s_tab[];
    bool bad = false;
    for (int pg = (first >> 6) + (tid & 63); pg <= (pos >> 6); pg += 64) {
      const int e = a.table[pg];
      bad |= (unsigned)e >= (unsigned)a.n_pages;
      if (tid < 64) s_tab[pg] = e;
    }
    if (__any(bad)) {
      if (sidx == 0 && tid < HD) a.out[(size_t)h * HD + tid] = __builtin_bit_cast(f16, (unsigned short)0x7e00);
      return;
    }
    __syncthreads();
  }
  const float* cs = a.cos + (size_t)(pos - start) * HD;     // (start: 0 unless START)
  const float* sn = a.sin + (size_t)(pos - start) * HD;

  const f16* qh = a.q + (size_t)h * HD;
  const f16* kh = a.k + (size_t)kvh * HD;
  const f16* vh = a.v + (size_t)kvh * HD;
  // rotary factors of this thread's 8 dims (requested before the transforms: one memory round trip less)
  float c8[8], s8[8];
  if (tid < 256) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { c8[i] = cs[d0 + i]; s8[i] = sn[d0 + i]; }
  }
  if constexpr (ZIN) {
    extern __shared__ __attribute__((aligned(16))) float zbuf[];   // 3 x had::buf_floats(n)
    __shared__ __attribute__((aligned(16))) f16 s_qkv[3][HD];
    const bool act = zact;
    float v[16], tp[16];
    had::unpack8(zraw[0], v);
    had::unpack8(zraw[1], v + 8);
    had::unpack8(praw[0], tp);
    had::unpack8(praw[1], tp + 8);
    if constexpr (GQ) {
      // different lengths side by side: the shorter transform passes the barriers the longer one still has to meet
      float* zb = zbuf + (g3 == 0 ? 0 : had::buf_floats(1 << LQ) + (g3 - 1) * had::buf_floats(1 << LKV));
      if (g3 == 0) {
        had::fht16_fixed<LQ, false>(v, zb, 0, tt, true);
      } else {
        had::fht16_fixed<LKV, false>(v, zb, 0, tt, true);
#pragma unroll
        for (int i = 0; i < fht16_barriers(LQ) - fht16_barriers(LKV); ++i) __syncthreads();
      }
    } else {
      had::fht16(v, zbuf + g3 * had::buf_floats(zz.n), tt, zz.logL, act, 0);
    }
    const int base = (g3 == 0 ? h : kvh) * HD;
    if (act && e0 >= base && e0 < base + HD) {
      f16 o[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = had::out_elem(v[r], zz.scale[g3], true, tp[r], false, 0.f, false, 0.f);
      uint4* dst = reinterpret_cast<uint4*>(&s_qkv[g3][e0 - base]);
      dst[0] = *reinterpret_cast<uint4*>(&o[0]);
      dst[1] = *reinterpret_cast<uint4*>(&o[8]);
    }
    __syncthreads();
    if (tid >= 256) return;
    qh = s_qkv[0];
    kh = s_qkv[1];
    vh = s_qkv[2];
  }
  float q8[8], kn[8], vn[8];
  if constexpr (NORM) {
    // every lane group holds the whole head (and every split workgroup its own copy): normalised in registers
    attn::rope8_norm<HD>(qh, a.qw, a.eps, c8, s8, d0, q8);
    attn::rope8_norm<HD>(kh, a.kw, a.eps, c8, s8, d0, kn);
  } else {
    attn::rope8<HD>(qh, c8, s8, d0, q8);
    attn::rope8<HD>(kh, c8, s8, d0, kn);
  }
  const uint4 vraw = *reinterpret_cast<const uint4*>(vh + d0);
  attn::unpack8h(vraw, vn);
  // fp8: the row as stored -- its bytes, and in kn / vn the values those bytes mean
  uint2 knq{}, vnq{};
  float ksc = 1.f, vsc = 1.f;
  if constexpr (FP8) {
    ksc = attn::exp2i(a.k_exp);
    vsc = attn::exp2i(a.v_exp);
    knq = attn::quant8f8(kn, attn::exp2i(-a.k_exp));
    vnq = attn::quant8f8(vn, attn::exp2i(-a.v_exp));
    attn::unpack8f8(knq, ksc, kn);
    attn::unpack8f8(vnq, vsc, vn);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) q8[i] *= a.scale;
  // row t of this head's KV head: contiguous, base + t rows; paged, row t & 63 of the head's part of page table[t >> 6]
  f16* kc = PAGED ? a.kcache : a.kcache + (size_t)kvh * a.max_len * HD;
  f16* vc = PAGED ? a.vcache : a.vcache + (size_t)kvh * a.max_len * HD;
  const auto row = [&](int t) -> size_t {
    if constexpr (PAGED) {
      extern __shared__ int s_tab[];
      return (((size_t)s_tab[t >> 6] * a.kv_heads + kvh) * kPage + (t & (kPage - 1))) * HD;
    } else {
      return (size_t)t * HD;
    }
  };
  if constexpr (FP8) {   // (row offsets count elements: bytes here)
    if (h % group == 0 && grp == 0 && sidx == 0) {
      *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(kc) + row(pos) + d0) = knq;
      *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(vc) + row(pos) + d0) = vnq;
    }
  } else if (h % group == 0 && grp == 0 && sidx == 0) {   // append the new row (StaticCache.update)
    uint4 kr;
    kr.x = pack_f16(kn[0], kn[1]); kr.y = pack_f16(kn[2], kn[3]);
    kr.z = pack_f16(kn[4], kn[5]); kr.w = pack_f16(kn[6], kn[7]);
    *reinterpret_cast<uint4*>(kc + row(pos) + d0) = kr;
    *reinterpret_cast<uint4*>(vc + row(pos) + d0) = vraw;
  }

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int t0 = t_lo + grp; t0 < t_hi; t0 += NG * U) {
    typename std::conditional<FP8, uint2, uint4>::type kr[U], vr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u * NG;
      // t == pos comes from registers, t > pos is masked: a dummy row (paged: one of a validated page; START: none below start)
      const int tc = t < pos ? t : (PAGED || START ? first : 0);
      if constexpr (FP8) {
        kr[u] = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(kc) + row(tc) + d0);
        vr[u] = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(vc) + row(tc) + d0);
      } else {
        kr[u] = *reinterpret_cast<const uint4*>(kc + row(tc) + d0);
        vr[u] = *reinterpret_cast<const uint4*>(vc + row(tc) + d0);
      }
    }
    // the round's scores first (independent chains), then the online-softmax updates in key order
    float k8a[U][8], v8a[U][8], sa[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u * NG;
      if constexpr (FP8) {
        attn::unpack8f8(kr[u], ksc, k8a[u]);
        attn::unpack8f8(vr[u], vsc, v8a[u]);
      } else {
        attn::unpack8h(kr[u], k8a[u]);
        attn::unpack8h(vr[u], v8a[u]);
      }
      if (t == pos) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { k8a[u][i] = kn[i]; v8a[u][i] = vn[i]; }
      }
      sa[u] = attn::score<LPK>(q8, k8a[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u * NG;
      const float s = sa[u];
      const float (&v8)[8] = v8a[u];
      if (t < t_hi) {
        // attn::update, written out (as a call it moved the registers and the schedule of every instantiation)
        const float mn = fmaxf(m, s);
        const float c = __expf(m - mn), p = __expf(s - mn);
        l = __builtin_fmaf(l, c, p);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(acc[i], c, had::fmul(p, v8[i]));
        m = mn;
      }
    }
  }
  if (gl == 0) { s_m[grp] = m; s_l[grp] = l; }
#pragma unroll
  for (int i = 0; i < 8; ++i) s_acc[grp][d0 + i] = acc[i];
  __syncthreads();
  float M = -INFINITY, Lsum = 0.f, o = 0.f;
  if (tid < HD) {
    // attn::merge_states, written out (s_m / s_l / s_acc are LDS arrays here: read through pointers they were scheduled
    // differently)
    for (int g = 0; g < NG; ++g) M = fmaxf(M, s_m[g]);
    for (int g = 0; g < NG; ++g) {
      const float w = s_m[g] == -INFINITY ? 0.f : __expf(s_m[g] - M);
      Lsum = __builtin_fmaf(s_l[g], w, Lsum);
      o = __builtin_fmaf(s_acc[g][tid], w, o);
    }
  }
  if (!split) {
    if (tid < HD) a.out[(size_t)h * HD + tid] = (f16)(o / Lsum);
    return;
  }
  // Publish this split's state, then count arrivals; the last one merges.  The exchange uses
  // agent-scope atomic stores / loads (coherent across the XCDs' L2s by themselves) ordered by
  // "all my stores have completed" (s_waitcnt vmcnt(0)) -> barrier -> counter increment, instead of
  // __threadfence(): a release fence writes back the whole L2, measured ~20 us per launch here.
  float* mine = a.ws + ((size_t)h * kSplits + sidx) * (HD + 4);
  if (tid < HD) __hip_atomic_store(mine + tid, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) {
    __hip_atomic_store(mine + HD, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(mine + HD + 1, Lsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __shared__ unsigned s_old;
  __syncthreads();
  if (tid == 0) s_old = __hip_atomic_fetch_add(a.counters + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (s_old != kSplits - 1) return;
  asm volatile("" ::: "memory");
  if (tid < HD) {
    float* base = a.ws + (size_t)h * kSplits * (HD + 4);
    float ms[kSplits], ls[kSplits], os[kSplits];
#pragma unroll
    for (int s2 = 0; s2 < kSplits; ++s2) {
      ms[s2] = __hip_atomic_load(base + s2 * (HD + 4) + HD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ls[s2] = __hip_atomic_load(base + s2 * (HD + 4) + HD + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      os[s2] = __hip_atomic_load(base + s2 * (HD + 4) + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float Mx = -INFINITY;                              // attn::merge_states, written out (as a call: other registers)
#pragma unroll
    for (int s2 = 0; s2 < kSplits; ++s2) Mx = fmaxf(Mx, ms[s2]);
    float L2 = 0.f, o2 = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < kSplits; ++s2) {
      const float w = ms[s2] == -INFINITY ? 0.f : __expf(ms[s2] - Mx);
      L2 = __builtin_fmaf(ls[s2], w, L2);
      o2 = __builtin_fmaf(os[s2], w, o2);
    }
    a.out[(size_t)h * HD + tid] = (f16)(o2 / L2);
  }
  if (tid == 0) __hip_atomic_store(a.counters + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next launch
}

}  // namespace

// ---- the host path of every attention launch of this translation unit ---------------------------------------------------
// Operands and sizes arrive as AttnIO / AttnShape (quip_internal.h).  make_attn_args / make_chunk_args are the one place
// where they become kernel arguments, place_workspace the one place of the split rule and of the workspace layout,
// decode_launch the one launch of the decode-side kernels without _z input.  A launcher is its shape checks (BAD_SHAPE
// before UNSUPPORTED), what its argument type adds, and one call.
namespace {

AttnArgs make_attn_args(const AttnIO& io, const AttnShape& s) {
  return AttnArgs{reinterpret_cast<const f16*>(io.q), reinterpret_cast<const f16*>(io.k), reinterpret_cast<const f16*>(io.v),
                  io.cos, io.sin, io.pos, reinterpret_cast<f16*>(io.kcache), reinterpret_cast<f16*>(io.vcache),
                  reinterpret_cast<f16*>(io.out), s.heads, s.kv_heads, s.max_len, s.scale, nullptr, nullptr, s.window};
}

// one of the types derived from AttnArgs with its base filled; the caller sets what the type adds
template <class Args>
Args make_attn_args_as(const AttnIO& io, const AttnShape& s) {
  Args a{};
  static_cast<AttnArgs&>(a) = make_attn_args(io, s);
  return a;
}

// what every launch asks of its sizes; the batched ones add batch_ok, the paged ones paged_shape_ok (paged_attn.hip.h)
bool attn_shape_ok(const AttnShape& s) {
  return s.heads >= 1 && s.kv_heads >= 1 && s.heads % s.kv_heads == 0 && s.max_len >= 1;
}
bool batch_ok(int batch) { return batch >= 1 && batch <= 65535; }       // grid.z

// Split mode: a workspace is given and the cache can hold a context beyond kSplitFromPos (`len`: max_len, or what the
// block table can address).  The workspace: partial states of every (sequence, head, split), then the arrival counters
// of every (sequence, head).  -> whether the launch is split (grid.y = kSplits)
bool place_workspace(AttnArgs& a, int batch, int head_dim, long long len, void* workspace) {
  if (workspace == nullptr || len <= kSplitFromPos) return false;
  a.ws = reinterpret_cast<float*>(workspace);
  a.counters = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(workspace) +
                                           (size_t)batch * a.heads * kSplits * (head_dim + 4) * sizeof(float));
  return true;
}

// The decode-side launch on filled arguments: SEQ false is the bs = 1 kernel (batch 1), true the batched one.
template <bool SEQ, class Args>
int decode_launch(Args a, int batch, int head_dim, long long split_len, int lds, hipStream_t stream, void* workspace) {
  const bool split = place_workspace(a, batch, head_dim, split_len, workspace);
  const dim3 grid(a.heads, split ? kSplits : 1, batch);
  const AttnZ none{};
  if (head_dim == 128)
    return launch<rope_attn_decode_kernel<128, false, 0, 0, SEQ, Args>>(grid, dim3(256), lds, stream, a, none);
  if (head_dim == 64)
    return launch<rope_attn_decode_kernel<64, false, 0, 0, SEQ, Args>>(grid, dim3(256), lds, stream, a, none);
  return QUIP_ERR_UNSUPPORTED;
}

}  // namespace

size_t rope_attn_workspace_bytes(int heads, int head_dim) {
  return (size_t)heads * kSplits * (head_dim + 4) * sizeof(float) + (size_t)heads * sizeof(unsigned);
}

size_t rope_attn_batched_workspace_bytes(int batch, int heads, int head_dim) {
  return (size_t)batch * rope_attn_workspace_bytes(heads, head_dim);
}

bool rope_attn_decode_z_supported(int heads, int kv_heads, int head_dim) {
  const int n = heads * head_dim;
  // grouped queries: Llama-2-70B / Llama-3-70B (64 heads, 8 KV heads) and Llama-3-8B / Mistral-7B (32 / 8)
  if (heads != kv_heads) return head_dim == 128 && kv_heads == 8 && (heads == 64 || heads == 32);
  return heads >= 1 && (head_dim == 64 || head_dim == 128) && n >= 256 && n <= 4096 && (n & (n - 1)) == 0;
}

// The _z launch chooses its own instance (transform widths, block size, LDS); workspace and grid are the bs = 1 launch's.
int rope_attn_decode_z_launch(const void* const* z, const void* const* post, const float* scales, const AttnIO& io,
                              const AttnShape& s, hipStream_t stream, void* workspace) {
  if (s.heads < 1 || s.kv_heads < 1 || s.max_len < 1) return QUIP_ERR_BAD_SHAPE;
  if (!rope_attn_decode_z_supported(s.heads, s.kv_heads, s.head_dim)) return QUIP_ERR_UNSUPPORTED;
  AttnArgs a = make_attn_args(io, s);
  AttnZ zz{};
  const int head_dim = s.head_dim, nq = s.heads * head_dim, nkv = s.kv_heads * head_dim;
  for (int i = 0; i < 3; ++i) {
    zz.z[i] = reinterpret_cast<const f16*>(z[i]);
    zz.post[i] = reinterpret_cast<const f16*>(post[i]);
    zz.scale[i] = scales[i];
  }
  zz.n = nq;
  zz.logL = 31 - __builtin_clz((unsigned)nq);
  const dim3 grid(s.heads, place_workspace(a, 1, head_dim, s.max_len, workspace) ? kSplits : 1);
  if (s.heads != s.kv_heads) {
    const size_t lds = ((size_t)had::buf_floats(nq) + 2 * (size_t)had::buf_floats(nkv)) * sizeof(float);
    if (head_dim == 128 && nq == 8192 && nkv == 1024)
      return launch<rope_attn_decode_kernel<128, true, 13, 10>>(grid, dim3(512 + 128), (int)lds, stream, a, zz);
    if (head_dim == 128 && nq == 4096 && nkv == 1024)
      return launch<rope_attn_decode_kernel<128, true, 12, 10>>(grid, dim3(256 + 128), (int)lds, stream, a, zz);
    return QUIP_ERR_UNSUPPORTED;
  }
  const size_t lds = 3 * (size_t)had::buf_floats(nq) * sizeof(float);
  if (head_dim == 128) return launch<rope_attn_decode_kernel<128, true>>(grid, dim3(768), (int)lds, stream, a, zz);
  if (head_dim == 64) return launch<rope_attn_decode_kernel<64, true>>(grid, dim3(768), (int)lds, stream, a, zz);
  return QUIP_ERR_UNSUPPORTED;
}

int rope_attn_decode_launch(const AttnIO& io, const AttnShape& s, hipStream_t stream, void* workspace) {
  if (!attn_shape_ok(s)) return QUIP_ERR_BAD_SHAPE;
  return decode_launch<false>(make_attn_args(io, s), 1, s.head_dim, s.max_len, 0, stream, workspace);
}

int rope_attn_decode_batched_launch(const AttnIO& io, const AttnShape& s, hipStream_t stream, void* workspace) {
  if (!batch_ok(s.batch) || !attn_shape_ok(s)) return QUIP_ERR_BAD_SHAPE;
  return decode_launch<true>(make_attn_args(io, s), s.batch, s.head_dim, s.max_len, 0, stream, workspace);
}

int rope_attn_decode_batched_start_launch(const AttnIO& io, const int64_t* start, const AttnShape& s, hipStream_t stream,
                                          void* workspace) {
  if (!batch_ok(s.batch) || !attn_shape_ok(s)) return QUIP_ERR_BAD_SHAPE;
  auto a = make_attn_args_as<StartAttnArgs>(io, s);
  a.start = start;
  return decode_launch<true>(a, s.batch, s.head_dim, s.max_len, 0, stream, workspace);
}

// Greedy tail of the decode step (example_generate.py's argmax sampling with temperature 0): next token =
// first index of the largest logit (torch.argmax's tie rule), stored to tok; pos += 1.  One workgroup per row of
// (rows, n) logits -- row r sets tok[r] and advances pos[r]; the bs=1 tail is one row: the three framework launches it
// replaces (reduce, copy, add) cost ~20 us of a 2.5 ms token.  The first index of the maximum does not depend on the
// order of the scan, so rows whose start is not 16-byte aligned (odd n) take 2-byte loads and give the same token.
// (The rule is argmax_better, quip_device.hip.h; this kernel and nll_rows.hip.h spell it out: called as a function the
// comparisons compile to other code.)
namespace {
__global__ __launch_bounds__(1024) void argmax_step_kernel(const f16* __restrict__ logits, int n,
                                                           int64_t* __restrict__ tok, int64_t* __restrict__ pos) {
  __shared__ float sv[16];
  __shared__ int si[16];
  const int tid = threadIdx.x;
  logits += (size_t)blockIdx.x * n;
  tok += blockIdx.x;
  pos += blockIdx.x;
  const bool vec = (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  float best = -3.0e38f;
  int bi = 0x7fffffff;
  for (int i = tid * 8; i < n; i += 1024 * 8) {
    if (vec && i + 8 <= n) {
      const uint4 q = *reinterpret_cast<const uint4*>(logits + i);
      const f16* h = reinterpret_cast<const f16*>(&q);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = (float)h[j];
        if (v > best || (v == best && i + j < bi)) { best = v; bi = i + j; }
      }
    } else {
      for (int j = i; j < min(n, i + 8); ++j) {
        const float v = (float)logits[j];
        if (v > best || (v == best && j < bi)) { best = v; bi = j; }
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w)
      if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
    // (all-NaN / all -inf logits -- e.g. the answer of a persistent launch that gave up -- leave no index: token 0, a
    //  valid row of the embedding table, instead of INT_MAX into the next step's lookup)
    tok[0] = bi < n ? bi : 0;
    pos[0] += 1;
  }
}
}  // namespace

int argmax_step_launch(const void* logits, int n, void* tok, void* pos, hipStream_t stream) {
  if (n < 1) return QUIP_ERR_BAD_SHAPE;
  return launch<argmax_step_kernel>(dim3(1), dim3(1024), 0, stream, reinterpret_cast<const f16*>(logits), n,
                                    reinterpret_cast<int64_t*>(tok), reinterpret_cast<int64_t*>(pos));
}

int argmax_step_batched_launch(const void* logits, int batch, int n, void* tok, void* pos, hipStream_t stream) {
  if (batch < 1 || n < 1) return QUIP_ERR_BAD_SHAPE;
  return launch<argmax_step_kernel>(dim3(batch), dim3(1024), 0, stream, reinterpret_cast<const f16*>(logits), n,
                                    reinterpret_cast<int64_t*>(tok), reinterpret_cast<int64_t*>(pos));
}

}  // namespace quip

// the prompt-side launches: rope + cache append + causal attention for a chunk of rows, for a ragged batch of chunks
#include "chunk_attn.hip.h"
#include "ragged_attn.hip.h"
// both batched launches on a paged cache: rows addressed through a block table
#include "paged_attn.hip.h"
// per-head RMSNorm of q / k (Qwen3): the stand-alone launch and the launchers of the kNorm instantiations
#include "qk_norm.hip.h"
// the scoring tail: log-sum-exp, target log-probability and arg-max of every row of a chunk's logits
#include "nll_rows.hip.h"
// the sampling tail: one token per row, every row with its own temperature, top-k, top-p and seed
#include "sample_rows.hip.h"
// speculative greedy decode: accept the confirmed guesses of a chunk pass, emit, rewind, draft the next ones by prompt lookup
#include "spec_rows.hip.h"
// LoRA adapters beside the quantised modules, one adapter index per row: the shrink and the expand launch
#include "lora_rows.hip.h"
