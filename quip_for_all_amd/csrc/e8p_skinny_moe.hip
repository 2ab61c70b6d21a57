// The routed skinny product of a sparse-MoE MLP at decode rows (1 <= M <= 31 tokens), gfx950, E8P12:
//
//   Y[g][s, :] = fp16(scale[g, e(s)] * fp16(X[g][s, :] . decode(Q[g][e(s)])^T)),   g < G <= 2 (gate and up, or down alone)
//
// Q[g] stacks the E <= 64 experts' codes, (E, n, k / 8); the P = M top_k rows of X[g] are sorted by expert and expert e owns
// rows [start[e], start[e + 1]).  `start` is device memory written by moe_route_rows_kernel (moe_rows.hip.h): the host names
// no expert, reads nothing back, and a captured launch serves whatever experts later inputs select.
//
// Mapping: that of e8p_skinny_group.hip -- a TILE is 32 CB columns of one (g, expert), the grid is min(G E column tiles, CUs)
// workgroups of 160 KB LDS, each builds the decode tables once and walks tiles b, b + gridDim.x, ...; the tile body is
// e8p_skinny_tile.hip.h (WALK = 2).  What a grouped tile takes from the kernel arguments a routed tile reads on the device:
// its row count M_e = start[e + 1] - start[e], its row base X[g] + start[e] k and its code base Q[g] + e n k / 8 (scalar
// loads at the top of the tile, clamped into the P rows whatever `start` holds).
// Tile order: only experts that own rows have tiles.  Every workgroup ballots the E row counts once (lane e: expert e) and
// numbers the tiles (g, j-th non-empty expert, column tile) with the column tile fastest.  Empty experts are never
// enumerated, so nothing of them is requested -- at M = 1, top_k = 2 of 8 experts a quarter of the codes stream -- and the
// walk stays balanced: every tile streams the same 32 CB k / 4 bytes of codes (the rows ride along in L2), the numbering is
// dense, so workgroups differ by at most one tile.  Column tile fastest keeps neighbouring workgroups on one expert's rows
// of X and on adjacent code rows.  The grid is sized on the host for all E experts; workgroups beyond the tiles that exist
// leave before they request anything.
// MP (rows staged per granule) is chosen from M on the host: M_e <= M.  CB is the single launch's choice for n, so the K
// slices are added in the single launch's order: before the scale, row s of Y[g] is bit for bit e8p_mm_skinny on
// (X[g][start[e] : start[e + 1]], Q[g][e]).  The scale (w_scale of the module, which the transform in front can no longer
// carry because a launch mixes modules) multiplies that fp16 value in fp32 and is rounded once more.
// The other four codebooks: their code rows have other strides; refused (QUIP_ERR_UNSUPPORTED) until somebody needs them.
#include "e8p_skinny_tile.hip.h"
#include "moe_rows.hip.h"

namespace quip {

namespace {

template <int CB, int MP>
__global__ __launch_bounds__(1024) void e8p_skinny_moe_kernel(const SkinnyMoeArgs ma, int K, const uint64_t* __restrict__ grid) {
  skinny_tiles<CB, MP, 0, 2>(nullptr, nullptr, grid, nullptr, 0, 0, K, 0.f, nullptr, 0, nullptr, &ma);
}

}  // namespace

int skinny_moe_launch(CodebookId cb, const void* x, const void* const* qidxs, const void* grid, const float* scale,
                      const int32_t* start, void* y, int count, int experts, int m, int pairs, int n, int k,
                      hipStream_t stream) {
  if (cb != kE8P) return QUIP_ERR_UNSUPPORTED;
  if (count < 1 || count > 2 || experts < 1 || experts > kMoeMaxExperts || m < 1 || m > kMoeMaxRows || pairs < m ||
      pairs > m * kMoeMaxTopK)
    return QUIP_ERR_UNSUPPORTED;
  if (!e8p_skinny_gemm_supported(m, n, k)) return QUIP_ERR_UNSUPPORTED;
  const bool one = skinny_group_one_block(n);
  SkinnyMoeArgs ma;
  ma.x = reinterpret_cast<const f16*>(x);
  ma.q[0] = reinterpret_cast<const uint16_t*>(qidxs[0]);
  ma.q[1] = reinterpret_cast<const uint16_t*>(qidxs[count - 1]);
  ma.y = reinterpret_cast<f16*>(y);
  ma.start = start;
  ma.scale = scale;
  ma.G = count;
  ma.E = experts;
  ma.P = pairs;
  ma.N = n;
  ma.M = m;
  const int cols = one ? 32 : 64;
  const long long tiles = (long long)count * experts * ((n + cols - 1) / cols);
  const int cus = device_cu_count();
  const uint64_t* gp = reinterpret_cast<const uint64_t*>(grid);
  auto go = [&](auto kern) -> int {
    return launch<decltype(kern)::value>(dim3((unsigned)(tiles < cus ? tiles : cus)), dim3(1024), kSLds, stream, ma, k, gp);
  };
  if (m <= 16) return one ? go(kernel_c<e8p_skinny_moe_kernel<1, 16>>) : go(kernel_c<e8p_skinny_moe_kernel<2, 16>>);
  return one ? go(kernel_c<e8p_skinny_moe_kernel<1, 32>>) : go(kernel_c<e8p_skinny_moe_kernel<2, 32>>);
}

}  // namespace quip
