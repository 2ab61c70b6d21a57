// The two batched attention launches on a PAGED KV cache (part of decode_glue.hip's translation unit).
//
// Layout.  A page is kPage = 64 consecutive positions of every KV head of one sequence -- exactly one key tile of the
// prompt-side launch (kPage == kChunkTile).  Per layer one pool for K and one for V, fp16 (n_pages, kv_heads, 64, HD):
// one KV head's part of a page is 64 HD contiguous values.  The block table, int32 (B, max_pages), contiguous, on the
// device, names the page of positions [64 j, 64 j + 64) of slot b in entry [b][j]; -1 is "none".  Row t of KV head g of
// slot b:  pool + ((table[b][t >> 6] * kv_heads + g) * 64 + (t & 63)) * HD.
//
// rope_attn_decode_paged_launch is rope_attn_decode_batched_launch and rope_attn_ragged_paged_launch is
// rope_attn_ragged_launch with that address in place of the contiguous one: the kernels are the same templates
// (rope_attn_decode_kernel over PagedAttnArgs, chunk_tile_body over PagedChunkArgs), so the walk, the split rule, the
// window rule, taking the new rows from registers / the inputs and all arithmetic are shared text.  Hence the oracle:
// a paged launch is BIT IDENTICAL, outputs and cache rows, to the contiguous launch on the rows gathered through the
// table.  The decode launch brings the sequence's table row into LDS once per workgroup (the key loop's loads depend
// on an LDS read, not on a second global load); the ragged launch looks up one page per key tile, wave uniform.
//
// Table validity is part of the range rule -- a bad entry never becomes an address:
//   decode: an entry of pages first >> 6 .. pos >> 6 outside [0, n_pages) -> nothing appended, the sequence's heads NaN
//           (first: the window's first key, 0 without a window);
//   ragged: the same for pages kfirst >> 6 .. (pos + rows - 1) >> 6 of a segment (kfirst: first key of its first row)
//           -> that segment's rows NaN, nothing appended to it, the other segments keep their bits.
// Every workgroup of a sequence / segment scans the same entries and reaches the same verdict: no partial append.
// Entries below a window's first page are not examined (they may have been released).
//
// HOST INVARIANT, not checked on the device: a page that any slot of the launch appends to is referenced by that slot
// only.  Rule (1) of chunk_attn.hip.h (no workgroup reads a cache row another workgroup of the launch writes) then
// holds across slots that share read-only prefix pages: shared pages are read by several slots and written by none.
//
// FP8 POOLS (the _f8 launches).  The same two launches on pools of one byte per element, uint8 (n_pages, kv_heads, 64,
// HD): a stored byte c of the K pool means e4m3fn(c) * 2^k_exp, of the V pool e4m3fn(c) * 2^v_exp (OCP e4m3fn; one
// power-of-two scale per pool, by value in the launch arguments, an integer in [-8, 7]: every code times 2^e is then an
// exact, finite fp16 value, so dequantisation is exact).  Same table, same pages, same walks: the kernels are the paged
// templates over PagedAttnArgsF8 / PagedChunkArgsF8.  A cached row is loaded as 8 bytes per lane / chunk and converted
// to the values the fp16 kernels unpack; from there on the arithmetic is theirs, so an fp8 launch is BIT IDENTICAL, in
// its outputs, to the fp16 paged launch on pools that hold the dequantised bytes whenever the new rows are
// representable.  Appending quantises: x * 2^-e in fp32 (exact), finite values beyond +-448 and +-inf saturate to +-448
// (explicitly, by compares), NaN stays NaN ((byte & 0x7f) == 0x7f), the rest rounds to nearest even, subnormals included.
// THE ROUND-TRIP RULE: the rows a launch appends are used BY THAT LAUNCH as dequant(quant(.)) -- the decode kernel
// replaces the new key and value before t == pos is scored, the chunk body stages every own-chunk row that way and
// stores exactly those bytes.  "The bits of the cached row" (rule (1) of chunk_attn.hip.h) stays true, a row's result
// does not depend on whether its keys were found in the cache or in the launch's inputs, and rule (2) -- any split of
// a chunk into consecutive launches gives the same bits -- keeps holding.
#pragma once
#include "chunk_attn.hip.h"
#include "ragged_attn.hip.h"

namespace quip {
namespace {

static_assert(kPage == kChunkTile, "a page is one key tile of the prompt-side launch");
constexpr int kPagedMaxPages = 8192;     // the decode launch keeps a table row in LDS: 32 KiB, 524288 positions

struct PagedRaggedArgs {
  PagedChunkArgs c;   // as RaggedArgs::c; kcache / vcache: the pools, table: row 0 of the block table
  int nseg;
  int slot[kRaggedMaxSegments], row0[kRaggedMaxSegments], rows[kRaggedMaxSegments];
};

template <int HD>
__global__ __launch_bounds__(kChunkThreads) void rope_attn_paged_ragged_kernel(PagedRaggedArgs ra) {
  // the segment scan of the contiguous ragged launch (ragged_attn.hip.h)
  int s = 0, t0 = 0;
  for (; s < ra.nseg - 1; ++s) {
    const int n = (ra.rows[s] + kChunkTile - 1) / kChunkTile;
    if ((int)blockIdx.y < t0 + n) break;
    t0 += n;
  }
  const int slot = ra.slot[s];
  const size_t r0 = (size_t)ra.row0[s];
  PagedChunkArgs a = ra.c;
  a.q += r0 * a.heads * HD;
  a.out += r0 * a.heads * HD;
  a.k += r0 * a.kv_heads * HD;
  a.v += r0 * a.kv_heads * HD;
  a.table += (size_t)slot * a.max_pages;
  a.pos += slot;
  a.rows = ra.rows[s];
  chunk_tile_body<HD>(a, (int)blockIdx.y - t0);
}

struct PagedRaggedArgsF8 {
  PagedChunkArgsF8 c;
  int nseg;
  int slot[kRaggedMaxSegments], row0[kRaggedMaxSegments], rows[kRaggedMaxSegments];
};

// rope_attn_paged_ragged_kernel on fp8 pools: the same scan in front of chunk_tile_body over PagedChunkArgsF8
template <int HD>
__global__ __launch_bounds__(kChunkThreads) void rope_attn_paged_ragged_f8_kernel(PagedRaggedArgsF8 ra) {
  int s = 0, t0 = 0;
  for (; s < ra.nseg - 1; ++s) {
    const int n = (ra.rows[s] + kChunkTile - 1) / kChunkTile;
    if ((int)blockIdx.y < t0 + n) break;
    t0 += n;
  }
  const int slot = ra.slot[s];
  const size_t r0 = (size_t)ra.row0[s];
  PagedChunkArgsF8 a = ra.c;
  a.q += r0 * a.heads * HD;
  a.out += r0 * a.heads * HD;
  a.k += r0 * a.kv_heads * HD;
  a.v += r0 * a.kv_heads * HD;
  a.table += (size_t)slot * a.max_pages;
  a.pos += slot;
  a.rows = ra.rows[s];
  chunk_tile_body<HD>(a, (int)blockIdx.y - t0);
}

bool fp8_exp_ok(int e) { return e >= -8 && e <= 7; }

// what the paged launches ask beyond attn_shape_ok (the launches on fp16 pools carry exponents 0)
bool paged_shape_ok(int max_len, const AttnPages& p) {
  return p.n_pages >= 1 && p.max_pages >= 1 && max_len >= 1 && (long long)max_len <= (long long)p.max_pages * kPage &&
         fp8_exp_ok(p.k_exp) && fp8_exp_ok(p.v_exp);
}

// what PagedAttnArgs / PagedChunkArgs and their F8 types add to their base
template <class Args>
void set_pages(Args& a, const AttnPages& p) {
  a.table = p.table;
  a.n_pages = p.n_pages;
  a.max_pages = p.max_pages;
  if constexpr (Args::kFp8) {     // (kcache / vcache carry the byte pools: the fp8 code addresses them as bytes)
    a.k_exp = p.k_exp;
    a.v_exp = p.v_exp;
  }
}

// rope_attn_decode_batched_launch on Args = PagedAttnArgs / PagedAttnArgsF8: the sequence's table row in dynamic LDS, and
// the split rule on what the table can address in place of max_len
template <class Args>
int decode_paged_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, hipStream_t stream, void* workspace) {
  if (!batch_ok(s.batch) || !attn_shape_ok(s) || !paged_shape_ok(s.max_len, pages)) return QUIP_ERR_BAD_SHAPE;
  if ((s.head_dim != 64 && s.head_dim != 128) || pages.max_pages > kPagedMaxPages) return QUIP_ERR_UNSUPPORTED;
  auto a = make_attn_args_as<Args>(io, s);
  set_pages(a, pages);
  return decode_launch<true>(a, s.batch, s.head_dim, (long long)pages.max_pages * kPage,
                             pages.max_pages * (int)sizeof(int32_t), stream, workspace);
}

// rope_attn_ragged_launch on RA = PagedRaggedArgs / PagedRaggedArgsF8 and its kernels
template <auto K128, auto K64, class RA>
int ragged_paged_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, int rows, const AttnSegments& segs,
                        hipStream_t stream) {
  if (!ragged_shape_ok(s, rows, segs.nseg) || !paged_shape_ok(s.max_len, pages)) return QUIP_ERR_BAD_SHAPE;
  RA ra{};
  static_cast<ChunkArgs&>(ra.c) = make_chunk_args(io, s, 0);
  set_pages(ra.c, pages);
  return ragged_launch<K128, K64>(ra, segs, s, rows, stream);
}

}  // namespace

int rope_attn_decode_paged_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, hipStream_t stream,
                                  void* workspace) {
  return decode_paged_launch<PagedAttnArgs>(io, pages, s, stream, workspace);
}

int rope_attn_ragged_paged_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, int rows,
                                  const AttnSegments& segs, hipStream_t stream) {
  return ragged_paged_launch<rope_attn_paged_ragged_kernel<128>, rope_attn_paged_ragged_kernel<64>, PagedRaggedArgs>(
      io, pages, s, rows, segs, stream);
}

// ---- the same two launches on fp8 pools (see the header of this file) ----------------------------------------------------
int rope_attn_decode_paged_f8_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, hipStream_t stream,
                                     void* workspace) {
  return decode_paged_launch<PagedAttnArgsF8>(io, pages, s, stream, workspace);
}

int rope_attn_ragged_paged_f8_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, int rows,
                                     const AttnSegments& segs, hipStream_t stream) {
  return ragged_paged_launch<rope_attn_paged_ragged_f8_kernel<128>, rope_attn_paged_ragged_f8_kernel<64>, PagedRaggedArgsF8>(
      io, pages, s, rows, segs, stream);
}

}  // namespace quip
