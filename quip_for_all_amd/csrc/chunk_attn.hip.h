// Prompt-side counterpart of rope_attn_decode_kernel (decode_glue.hip, whose translation unit this file is part of): rotary
// embedding, KV-cache append and causal softmax attention for a CHUNK of `rows` queries at positions [*pos, *pos + rows)
// against cache rows [0, *pos + rows), one launch.  q / out are token major ([rows, heads, HD], what the projections
// produce and o_proj consumes), the position is read on the device, so one captured launch serves every start position.
//
// One workgroup (two waves) per (64-row query tile, head); wave w owns query rows [32 w, 32 w + 32) of the tile.
//   * S^T = K Q^T (swapped product, v_mfma_f32_32x32x16_f16 with the key tile as A): the query row sits on the lane
//     (lane & 31), a lane and its partner lane ^ 32 hold the row's 64 scores of a key tile, 32 registers each -- the
//     online softmax is per lane, no cross-lane traffic beyond one exchange with the partner.
//   * The accumulator layout of S^T is the B operand layout of the next product, O^T = V^T P^T: registers 8 s .. 8 s + 7
//     rounded to fp16 are k-step s (element j of lane half h <-> key 16 s + 8 (j >> 2) + 4 h + (j & 3)); the matching A
//     operand (V^T) comes out of the row-major V tile through ds_read_b64_tr_b16.  O^T has the query row on the lane
//     again: the rescale of the running output is one multiplier per lane.
//   * K tile in LDS with the XOR swizzle (16-byte chunk c of key row r at c ^ (r % chunks)): the ds_read_b128 of the A
//     fragments (32 lanes, 32 different rows, one chunk column) spread over the banks.  V tile: plain rows padded by
//     64 bytes, so the four rows of a transposed-read block fall into four different bank groups.
//   * K / V are staged through registers (global -> VGPR -> LDS), one tile per barrier pair.
//
// Two rules shape the code:
//   (1) No workgroup reads a cache row that another workgroup of the launch writes.  Keys below *pos come from the
//       cache; keys of the chunk itself come from the k / v INPUTS and are rotated here by attn::rope8 -- the bits of the
//       cached row, as the decode launch takes key t == pos from registers.  Chunk row i is appended by exactly one
//       workgroup: the first query head of its KV group in the query tile that holds row i (which stages that key
//       anyway: a row attends to itself).
//   (2) A row's result depends on that row's q and on cache rows <= its position only.  Key tiles are aligned to
//       ABSOLUTE positions (tile j = keys [64 j, 64 j + 64), first and last masked per row), a tile that is masked
//       out entirely for a row leaves the row's state untouched bit for bit (p = 0, factor 1 or the -inf start), the
//       rescale is unconditional and per row, and an MFMA output column depends on its own B column only.  So any
//       split of a chunk into consecutive launches gives the same bits.
//
// Arithmetic: q and k rotated by attn::rope8 and rounded to fp16 (the decode launch's cache rows, bit for bit); scores
// fp32, the softmax scale applied to them in fp32; running max / sum fp32; P rounded to fp16 for P V; fp32
// accumulation; one rounding of the output to fp16.
//
// Range rule (the decode launch's, for the whole chunk): *pos < 0 or *pos + rows > max_len -> nothing is appended
// and every out row is NaN.
#pragma once
#include "attn_query.hip.h"
#include "launch.hip.h"
#include "quip_device.hip.h"

namespace quip {
namespace {

struct ChunkArgs {
  const f16* q;        // [rows, heads, HD]
  const f16* k;        // [rows, kv_heads, HD]  (pre-rope)
  const f16* v;        // [rows, kv_heads, HD]
  const float* cos;    // [max_len, HD]
  const float* sin;
  const int64_t* pos;  // device scalar: position of row 0
  f16* kcache;         // [kv_heads, max_len, HD]
  f16* vcache;
  f16* out;            // [rows, heads, HD]
  int rows;            // of the whole chunk (range rule), also when the launcher slices the grid
  int tile0;           // first query tile of this launch
  int heads, kv_heads, max_len, window;
  float scale;
  static constexpr bool kPaged = false;
  static constexpr bool kFp8 = false;
};

// A chunk on a PAGED cache (paged_attn.hip.h): kcache / vcache are page pools [n_pages, kv_heads, 64, HD], key tile j
// of the slot is page table[j].  max_len stays the row count of cos / sin and the bound of the range rule.
struct PagedChunkArgs : ChunkArgs {
  const int32_t* table;    // the slot's row of the block table: max_pages entries, -1: none
  int n_pages, max_pages;
  static constexpr bool kPaged = true;
};

// The same on pools of OCP e4m3fn bytes (one byte per element; a stored byte c means e4m3fn(c) * 2^k_exp in the K pool,
// e4m3fn(c) * 2^v_exp in the V pool).  A cached 8-byte chunk is converted to the 16-byte fp16 chunk that goes to LDS
// (exact); a row of the chunk itself is quantised, stored as those bytes and staged as dequant(quant(.)), so rule (1)'s
// "the bits of the cached row" and with it rule (2) keep holding.
struct PagedChunkArgsF8 : PagedChunkArgs {
  int k_exp, v_exp;        // in [-8, 7] (the launcher checks)
  static constexpr bool kFp8 = true;
};

typedef float cf32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 cf16x4 __attribute__((ext_vector_type(4)));

constexpr int kChunkTile = 64;        // query rows per workgroup == keys per tile
constexpr int kChunkThreads = 128;
constexpr int kChunkMaxTilesY = 65535;

// 4 keys x 16 dims of a row-major fp16 tile, transposed: lane i of a 16-lane group gets dim i of the four keys.  The
// wave must be whole (EXEC all ones): called from wave-uniform code only.
__device__ __forceinline__ cf16x4 lds_read_tr16(const unsigned char* p) {
  typedef __fp16 raw4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
  typedef raw4 __attribute__((address_space(3))) * lds_ptr;
  return __builtin_bit_cast(cf16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_ptr)(uintptr_t)p));
}

// One (64-row query tile, head) of a chunk: the whole body of the launch.  `tile` is the query tile inside the chunk
// `a` describes (wave uniform).  Shared, inlined, by rope_attn_chunk_kernel and the ragged launch (ragged_attn.hip.h),
// which points `a` at one segment of its rows first.  A: ChunkArgs, or PagedChunkArgs -- the same code with the cached
// rows of key tile jt read from, and the chunk's rows appended to, page table[jt] (one wave-uniform lookup per tile);
// or PagedChunkArgsF8, the paged code on byte pools (see the struct).  From LDS onwards nothing differs.
template <int HD, class A>
__device__ __forceinline__ void chunk_tile_body(const A& a, const int tile) {
  constexpr bool PAGED = A::kPaged;
  constexpr bool FP8 = A::kFp8;
  static_assert(!FP8 || PAGED, "the fp8 cache is a paged cache");
  constexpr int NCH = HD / 8;                       // 16-byte chunks per row
  constexpr int KROW = HD * 2, VROW = HD * 2 + 64;  // bytes per K / V row in LDS
  constexpr int NIT = kChunkTile * NCH / kChunkThreads;
  constexpr int KS = HD / 16, DB = HD / 32;
  __shared__ __attribute__((aligned(16))) unsigned char s_k[kChunkTile * KROW];
  __shared__ __attribute__((aligned(16))) unsigned char s_v[kChunkTile * VROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, i0 = tile * kChunkTile;
  const int nrow = min(kChunkTile, a.rows - i0);
  const int group = a.heads / a.kv_heads, kvh = h / group;
  const long long pos64 = *a.pos;
  bool refuse = pos64 < 0 || pos64 + (long long)a.rows > (long long)a.max_len;
  if constexpr (PAGED) {
    // Table validity, part of the range rule: the pages of the SEGMENT's keys, first key of its first row .. its last
    // row, whatever this workgroup's tile is -- every workgroup of the segment scans the same entries (each wave all
    // of them, one per lane and round) and reaches the same verdict.  Pages below the window's first are not looked at.
    if (!refuse) {
      const int p0 = (int)pos64;
      const int lo = a.window > 0 ? max(0, p0 + 1 - a.window) >> 6 : 0, hi = (p0 + a.rows - 1) >> 6;
      bool bad = false;
      for (int pg = lo + lane; pg <= hi; pg += 64) bad |= (unsigned)a.table[pg] >= (unsigned)a.n_pages;
      refuse = __any(bad);
    }
  }
  if (refuse) {
    const uint32_t nan2 = 0x7e007e00u;
    for (int e = tid; e < nrow * NCH; e += kChunkThreads)
      *reinterpret_cast<uint4*>(a.out + ((size_t)(i0 + e / NCH) * a.heads + h) * HD + (e % NCH) * 8) =
          make_uint4(nan2, nan2, nan2, nan2);
    return;
  }
  const int pos = (int)pos64;
  const int r = lane & 31, hh = lane >> 5;
  // rows behind the end of the chunk repeat its last row (never stored): every lane stays in range and in step
  const int qi = min(i0 + wave * 32 + r, a.rows - 1);
  const int my_p = pos + qi;
  const int my_first = a.window > 0 ? max(0, my_p + 1 - a.window) : 0;
  // the tile's keys: from the first key of its first row to the position of its last row
  const int p_hi = pos + i0 + nrow - 1;
  const int kfirst = a.window > 0 ? max(0, pos + i0 + 1 - a.window) : 0;
  const bool appender = h % group == 0;
  const f16* kc = a.kcache + (size_t)kvh * a.max_len * HD;      // (contiguous: this head's KV head, row 0)
  const f16* vc = a.vcache + (size_t)kvh * a.max_len * HD;
  float ksc = 1.f, vsc = 1.f, kisc = 1.f, visc = 1.f;      // fp8: 2^e and 2^-e of the two pools
  if constexpr (FP8) {
    ksc = attn::exp2i(a.k_exp), kisc = attn::exp2i(-a.k_exp);
    vsc = attn::exp2i(a.v_exp), visc = attn::exp2i(-a.v_exp);
  }
  // fp8: 8 stored bytes -> the fp16 chunk of the values they mean
  const auto chunk_of = [](const uint2& u, float sc) {
    float f[8];
    attn::unpack8f8(u, sc, f);
    return make_uint4(pack_f16(f[0], f[1]), pack_f16(f[2], f[3]), pack_f16(f[4], f[5]), pack_f16(f[6], f[7]));
  };

  // Q^T fragments (B operand): lane (r, hh) holds dims [16 ks + 8 hh, + 8) of its query row, rotated, fp16
  f16x8 qf[KS];
  {
    const f16* qrow = a.q + ((size_t)qi * a.heads + h) * HD;
    const float* cs = a.cos + (size_t)my_p * HD;
    const float* sn = a.sin + (size_t)my_p * HD;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int d0 = 16 * ks + 8 * hh;
      float c8[8], s8[8], o[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { c8[i] = cs[d0 + i]; s8[i] = sn[d0 + i]; }
      attn::rope8<HD>(qrow, c8, s8, d0, o);
#pragma unroll
      for (int i = 0; i < 8; ++i) qf[ks][i] = (f16)o[i];
    }
  }

  float m = -INFINITY, l = 0.f;
  cf32x16 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[db][g] = 0.f;

  for (int jt = kfirst / kChunkTile; jt <= p_hi / kChunkTile; ++jt) {
    // ---- stage keys [64 jt, 64 jt + 64): cache rows below *pos, the chunk's own rows from k / v (rotated here, and
    //      appended by the designated workgroup); rows no query of this tile attends to are zero
    uint4 kreg[NIT], vreg[NIT];
    size_t page0 = 0;     // paged: this KV head's part of the tile's page, row kr of it is key 64 jt + kr
    if constexpr (PAGED) page0 = ((size_t)a.table[jt] * a.kv_heads + kvh) * kChunkTile * HD;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = tid + kChunkThreads * it, kr = e / NCH, c = e % NCH, t = kChunkTile * jt + kr;
      uint4 kk = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
      if (t >= kfirst && t <= p_hi) {
        if (t < pos) {
          if constexpr (FP8) {      // (offsets count elements: bytes here)
            const size_t at = page0 + (size_t)kr * HD + c * 8;
            kk = chunk_of(*reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(a.kcache) + at), ksc);
            vv = chunk_of(*reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(a.vcache) + at), vsc);
          } else if constexpr (PAGED) {
            kk = *reinterpret_cast<const uint4*>(a.kcache + page0 + (size_t)kr * HD + c * 8);
            vv = *reinterpret_cast<const uint4*>(a.vcache + page0 + (size_t)kr * HD + c * 8);
          } else {
            kk = *reinterpret_cast<const uint4*>(kc + (size_t)t * HD + c * 8);
            vv = *reinterpret_cast<const uint4*>(vc + (size_t)t * HD + c * 8);
          }
        } else {
          const int i = t - pos;
          const f16* krow = a.k + ((size_t)i * a.kv_heads + kvh) * HD;
          const float* cs = a.cos + (size_t)t * HD + c * 8;
          const float* sn = a.sin + (size_t)t * HD + c * 8;
          float c8[8], s8[8], o[8];
#pragma unroll
          for (int x = 0; x < 8; ++x) { c8[x] = cs[x]; s8[x] = sn[x]; }
          attn::rope8<HD>(krow, c8, s8, c * 8, o);
          if constexpr (FP8) {
            float f[8];
            attn::unpack8h(*reinterpret_cast<const uint4*>(a.v + ((size_t)i * a.kv_heads + kvh) * HD + c * 8), f);
            const uint2 kq = attn::quant8f8(o, kisc), vq = attn::quant8f8(f, visc);
            kk = chunk_of(kq, ksc);
            vv = chunk_of(vq, vsc);
            if (appender && i >= i0) {
              const size_t at = page0 + (size_t)kr * HD + c * 8;
              *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(a.kcache) + at) = kq;
              *reinterpret_cast<uint2*>(reinterpret_cast<unsigned char*>(a.vcache) + at) = vq;
            }
          } else {
            kk.x = pack_f16(o[0], o[1]); kk.y = pack_f16(o[2], o[3]);
            kk.z = pack_f16(o[4], o[5]); kk.w = pack_f16(o[6], o[7]);
            vv = *reinterpret_cast<const uint4*>(a.v + ((size_t)i * a.kv_heads + kvh) * HD + c * 8);
            if (appender && i >= i0) {   // (i <= i0 + nrow - 1 by t <= p_hi): this tile's own rows
              const size_t at = PAGED ? page0 + (size_t)kr * HD : ((size_t)kvh * a.max_len + t) * HD;
              *reinterpret_cast<uint4*>(a.kcache + at + c * 8) = kk;
              *reinterpret_cast<uint4*>(a.vcache + at + c * 8) = vv;
            }
          }
        }
      }
      kreg[it] = kk;
      vreg[it] = vv;
    }
    __syncthreads();      // the previous tile's LDS reads are done
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int e = tid + kChunkThreads * it, kr = e / NCH, c = e % NCH;
      *reinterpret_cast<uint4*>(s_k + kr * KROW + 16 * (c ^ (kr & (NCH - 1)))) = kreg[it];
      *reinterpret_cast<uint4*>(s_v + kr * VROW + 16 * c) = vreg[it];
    }
    __syncthreads();

    // ---- S^T = K Q^T: s[kb][g] = score of key 64 jt + 32 kb + (g & 3) + 8 (g >> 2) + 4 hh for this lane's query row
    cf32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int g = 0; g < 16; ++g) s[kb][g] = 0.f;
      const int kr = 32 * kb + r;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(s_k + kr * KROW + 16 * ((2 * ks + hh) ^ (kr & (NCH - 1))));
        s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[kb], 0, 0, 0);
      }
    }
    // ---- scale in fp32, mask per row, online softmax per row (the partner lane holds the other 32 keys)
    float tmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int key = kChunkTile * jt + 32 * kb + (g & 3) + 8 * (g >> 2) + 4 * hh;
        const float x = (key <= my_p && key >= my_first) ? s[kb][g] * a.scale : -INFINITY;
        s[kb][g] = x;
        tmax = fmaxf(tmax, x);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);
    const float ms = mn == -INFINITY ? 0.f : mn;     // no key of the row so far: p = 0, the state stays (-inf, 0, 0)
    const float cf = __expf(m - ms);
    float psum = 0.f;
    f16x8 pf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const float p = __expf(s[kb][g] - ms);
        psum += p;
        pf[kb][g >> 3][g & 7] = (f16)p;
      }
    psum += __shfl_xor(psum, 32, 64);
    l = __builtin_fmaf(l, cf, psum);
    m = mn;
    // ---- O^T = O^T cf + V^T P^T
#pragma unroll
    for (int db = 0; db < DB; ++db) {
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[db][g] *= cf;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          // lane 4 q + p of a 16-lane group addresses key row q, dims [4 p, + 4) of the block; the group's block: keys
          // base + 4 hh + (0..3) (+ 8 for the fragment's upper half), dims 32 db + 16 (group & 1) + (0..15)
          const int key = 32 * kb + 16 * st + 4 * hh + ((lane & 15) >> 2);
          const unsigned char* vp = s_v + key * VROW + 2 * (32 * db + 16 * ((lane >> 4) & 1) + 4 * (lane & 3));
          const cf16x4 lo = lds_read_tr16(vp), hi = lds_read_tr16(vp + 8 * VROW);
          const f16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[kb][st], acc[db], 0, 0, 0);
        }
    }
  }
  // ---- out row = O / l, rounded once; lane (r, hh) holds dims 32 db + 8 gq + 4 hh + (0..3)
  if (i0 + wave * 32 + r < a.rows) {
    f16* orow = a.out + ((size_t)qi * a.heads + h) * HD;
    const float inv = 1.f / l;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        uint2 w;
        w.x = pack_f16(acc[db][4 * gq] * inv, acc[db][4 * gq + 1] * inv);
        w.y = pack_f16(acc[db][4 * gq + 2] * inv, acc[db][4 * gq + 3] * inv);
        *reinterpret_cast<uint2*>(orow + 32 * db + 8 * gq + 4 * hh) = w;
      }
  }
}

template <int HD>
__global__ __launch_bounds__(kChunkThreads) void rope_attn_chunk_kernel(ChunkArgs a) {
  chunk_tile_body<HD>(a, a.tile0 + (int)blockIdx.y);
}

// the kernel arguments of the prompt-side launches from AttnIO / AttnShape (quip_internal.h); rows: of the whole chunk,
// 0 where the kernel takes them per segment (the ragged launches)
ChunkArgs make_chunk_args(const AttnIO& io, const AttnShape& s, int rows) {
  return ChunkArgs{reinterpret_cast<const f16*>(io.q), reinterpret_cast<const f16*>(io.k), reinterpret_cast<const f16*>(io.v),
                   io.cos, io.sin, io.pos, reinterpret_cast<f16*>(io.kcache), reinterpret_cast<f16*>(io.vcache),
                   reinterpret_cast<f16*>(io.out), rows, 0, s.heads, s.kv_heads, s.max_len, s.window, s.scale};
}

// what the prompt-side launches ask of their sizes (attn_shape_ok: decode_glue.hip)
bool chunk_shape_ok(const AttnShape& s, int rows) { return rows >= 1 && attn_shape_ok(s) && s.window >= 0; }

}  // namespace

int rope_attn_chunk_launch(const AttnIO& io, const AttnShape& s, int rows, hipStream_t stream) {
  if (!chunk_shape_ok(s, rows)) return QUIP_ERR_BAD_SHAPE;
  const int heads = s.heads, head_dim = s.head_dim;
  if (head_dim != 64 && head_dim != 128) return QUIP_ERR_UNSUPPORTED;
  ChunkArgs a = make_chunk_args(io, s, rows);
  // query tiles on grid.y: more of them than one grid holds go out as slices of the same chunk (workgroups of a
  // launch never depend on each other, so neither do the slices)
  const int tiles = (rows - 1) / kChunkTile + 1;
  for (int t0 = 0; t0 < tiles; t0 += kChunkMaxTilesY) {
    a.tile0 = t0;
    const dim3 grid(heads, min(kChunkMaxTilesY, tiles - t0));
    const int rc = head_dim == 128 ? launch<rope_attn_chunk_kernel<128>>(grid, dim3(kChunkThreads), 0, stream, a)
                                   : launch<rope_attn_chunk_kernel<64>>(grid, dim3(kChunkThreads), 0, stream, a);
    if (rc != QUIP_OK) return rc;
  }
  return QUIP_OK;
}

}  // namespace quip
