// The chunk attention launch (chunk_attn.hip.h) for a RAGGED batch of
// chunks: S segments of consecutive rows of token-major q / k / v / out, segment s = seg_rows[s] rows that continue
// slot seg_slot[s] of a batched cache (B, kv_heads, max_len, HD) at the position the launch reads from pos[seg_slot[s]]
// (pos: the (B,) device counters of the batched decoder).  Per segment: rotary embedding, append to that slot's cache,
// causal (and windowed) attention over that slot's rows [0, pos + rows) -- chunk_tile_body, the code of
// rope_attn_chunk_kernel, unchanged.
//
// Grid (heads, sum_s ceil(seg_rows[s] / 64)): one workgroup per (64-row query tile of ONE segment, head); query tiles
// are per segment and never span two sequences.  The segment table (slot, first row, rows; <= kRaggedMaxSegments
// entries) travels by value in the kernel arguments: no device table, no host read of pos.  A workgroup finds its
// segment by scanning the cumulative tile counts (wave uniform, <= 32 steps, scalar loads from the argument segment),
// moves q / k / v / out to the segment's first row, kcache / vcache to the slot's slice and pos to the slot's entry,
// and runs the tile code.
//
// The two rules of chunk_attn.hip.h across segments:
//   (1) No workgroup reads a cache row another workgroup of the launch writes: within a segment by the chunk launch's
//       argument; across segments because the slots of one launch are DISTINCT (the host check refuses a slot named
//       twice), so two segments never touch the same cache slice.
//   (2) A row's result depends on its own q and on its slot's cache rows <= its position only.  Hence the oracle:
//       segment s's out rows and cache rows are bit identical to rope_attn_chunk run on that segment alone against
//       that slot's cache slice -- whatever the other segments are and in whatever order they come.
// Range rule, per segment: pos[slot] < 0 or pos[slot] + seg_rows[s] > max_len -> nothing is appended to that slot and
// that segment's out rows are NaN; every other segment is unaffected.
#pragma once
#include "chunk_attn.hip.h"
#include "launch.hip.h"

namespace quip {
namespace {

constexpr int kRaggedMaxSegments = QUIP_RAGGED_MAX_SEGMENTS;

struct RaggedArgs {
  ChunkArgs c;     // q / k / v / out at row 0 of the pass, kcache / vcache at slot 0, pos at entry 0; rows / tile0 unused
  int nseg;
  int slot[kRaggedMaxSegments], row0[kRaggedMaxSegments], rows[kRaggedMaxSegments];
};

template <int HD>
__global__ __launch_bounds__(kChunkThreads) void rope_attn_ragged_kernel(RaggedArgs ra) {
  // the segment of query tile blockIdx.y: the host made gridDim.y the total tile count, so the scan ends inside the table
  int s = 0, t0 = 0;
  for (; s < ra.nseg - 1; ++s) {
    const int n = (ra.rows[s] + kChunkTile - 1) / kChunkTile;
    if ((int)blockIdx.y < t0 + n) break;
    t0 += n;
  }
  const int slot = ra.slot[s];
  const size_t r0 = (size_t)ra.row0[s], slice = (size_t)slot * ra.c.kv_heads * ra.c.max_len * HD;
  ChunkArgs a = ra.c;
  a.q += r0 * a.heads * HD;
  a.out += r0 * a.heads * HD;
  a.k += r0 * a.kv_heads * HD;
  a.v += r0 * a.kv_heads * HD;
  a.kcache += slice;
  a.vcache += slice;
  a.pos += slot;
  a.rows = ra.rows[s];
  chunk_tile_body<HD>(a, (int)blockIdx.y - t0);
}

// The host side of a ragged launch on RA (RaggedArgs, or one of the paged ones of paged_attn.hip.h; ra.c is filled): the
// segment table -- distinct slots in [0, batch), every segment's first row, rows that sum to `rows` -- the grid of all
// segments' query tiles, and the launch of K128 / K64, the kernel over RA.
template <auto K128, auto K64, class RA>
int ragged_launch(RA& ra, const AttnSegments& g, const AttnShape& s, int rows, hipStream_t stream) {
  long long total = 0, tiles = 0;
  for (int i = 0; i < g.nseg; ++i) {
    if (g.rows[i] < 1 || g.slot[i] < 0 || g.slot[i] >= s.batch) return QUIP_ERR_BAD_SHAPE;
    for (int t = 0; t < i; ++t)
      if (g.slot[t] == g.slot[i]) return QUIP_ERR_BAD_SHAPE;     // rule (1) needs distinct slots
    if (total + g.rows[i] > rows) return QUIP_ERR_BAD_SHAPE;
    ra.slot[i] = g.slot[i];
    ra.row0[i] = (int)total;
    ra.rows[i] = g.rows[i];
    total += g.rows[i];
    tiles += (g.rows[i] - 1) / kChunkTile + 1;
  }
  if (total != rows) return QUIP_ERR_BAD_SHAPE;
  if (s.head_dim != 64 && s.head_dim != 128) return QUIP_ERR_UNSUPPORTED;
  if (tiles > kChunkMaxTilesY) return QUIP_ERR_UNSUPPORTED;           // callers chunk their passes
  ra.nseg = g.nseg;
  const dim3 grid(s.heads, (unsigned)tiles);
  return s.head_dim == 128 ? launch<K128>(grid, dim3(kChunkThreads), 0, stream, ra)
                           : launch<K64>(grid, dim3(kChunkThreads), 0, stream, ra);
}

// what the ragged launches ask of their sizes before the segments are looked at
bool ragged_shape_ok(const AttnShape& s, int rows, int nseg) {
  return nseg >= 1 && nseg <= kRaggedMaxSegments && s.batch >= 1 && chunk_shape_ok(s, rows);
}

}  // namespace

int rope_attn_ragged_launch(const AttnIO& io, const AttnShape& s, int rows, const AttnSegments& segs, hipStream_t stream) {
  if (!ragged_shape_ok(s, rows, segs.nseg)) return QUIP_ERR_BAD_SHAPE;
  RaggedArgs ra{};
  ra.c = make_chunk_args(io, s, 0);
  return ragged_launch<rope_attn_ragged_kernel<128>, rope_attn_ragged_kernel<64>>(ra, segs, s, rows, stream);
}

}  // namespace quip
