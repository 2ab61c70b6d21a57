// 1..3 skinny products in ONE launch: the q / k / v or gate / up projections of a decoder block at 2 <= M <= 32 rows, gfx950.
//
//   Y[g][m, n] = sum_k X[g][m, k] * W[g][n, k],   W[g] = decode(Qidxs[g]),   g < count <= 3, one M, K and codebook
//
// Why: the single launch (e8p_skinny_gemm.hip) is latency bound -- a workgroup requests its table source, builds 64 KB of
// decode tables, requests codes and granules and only then multiplies, for 32 or 64 columns; 4096 columns are 128
// workgroups on 256 CUs.  A block pays that chain once per module, on a machine that is half empty for q, k, v and o.
//
// Mapping: a TILE is the single launch's workgroup -- 32 CB columns of one problem, 16 waves = CB column blocks x 16 / CB
// slices of K.  The tiles of all problems are numbered through (problem g owns [tile0[g], tile0[g + 1])), the grid is
// min(tiles, CUs) workgroups (160 KB of LDS: one per CU), and workgroup b walks tiles b, b + gridDim.x, ...: q / k / v at
// 4096 is 384 tiles on 256 workgroups, gate / up at 11008 is 344.  The group travels by value in the kernel arguments;
// a tile's problem comes out of two scalar compares against the prefix.
//   per workgroup, once: the table source request and the table build (beside the first tile's code requests, as in the
//     single launch);
//   per tile: the body of e8p_skinny_tile.hip.h, unchanged -- the K slicing, the code loads and their v_permlane32_swap
//     relabelling, the ring of three row-contiguous granules per wave filled by global_load_lds_dwordx4, the hand-counted
//     vmcnt queue with its fillers, the K slices added in a fixed order through LDS.  So every Y[g] is bit identical to
//     the single launch on (X[g], Qidxs[g]);
//   between tiles: drain, barrier, reduce, barrier, then the next tile's prologue.  The sums are exchanged through the
//     rings' LDS, so no granule of the next tile may be requested before every wave has read its share; the second
//     barrier says so.  The next tile's code requests go out behind it as well (plain order: nothing of the next tile is
//     in flight across the reduction, no register in flight crosses the tile loop's edge).
// CB is the single launch's choice, a function of n alone, and fixes the order of the fp32 sums: a group whose problems
// disagree on it is refused (QUIP_ERR_UNSUPPORTED), the caller launches them one by one.  q / k / v take CB = 1, gate / up
// of the Llama shapes CB = 2.
// Bound: as the single launch -- LDS / L2 issue per tile; what the group saves is the table build and the first request
// round trip of every tile but a workgroup's first, and the idle CUs.
#include "e8p_skinny_tile.hip.h"

namespace quip {

namespace {

template <int CB, int MP, int MODE>
__global__ __launch_bounds__(1024) void e8p_skinny_group_kernel(const SkinnyGroupArgs ga) {
  skinny_tiles<CB, MP, MODE, true>(nullptr, nullptr, ga.grid, nullptr, ga.M, 0, ga.K, ga.resid_scale, ga.grid2, 0, &ga);
}

}  // namespace

// Refusals first, in the order of the single launch, then the tile prefix.  The branches below name the kernel
// instantiations, in the order of skinny_gemm_launch
int skinny_group_launch(CodebookId cb, const void* const* xs, const void* const* qidxs, const CodebookArgs& a, void* const* ys,
                        const int* ns, int count, int m, int k, hipStream_t stream) {
  if (count < 1 || count > 3 || m > 32) return QUIP_ERR_UNSUPPORTED;
  if (cb == kE8PRVQ3 && k % 32 != 0) return QUIP_ERR_UNSUPPORTED;      // rows of 3 k / 8 bytes, dword aligned
  for (int g = 0; g < count; ++g)
    if (!e8p_skinny_gemm_supported(m, ns[g], k)) return QUIP_ERR_UNSUPPORTED;
  const bool one = skinny_group_one_block(ns[0]);
  for (int g = 1; g < count; ++g)
    if (skinny_group_one_block(ns[g]) != one) return QUIP_ERR_UNSUPPORTED;
  const int cols = one ? 32 : 64;
  SkinnyGroupArgs ga;
  ga.tile0[0] = 0;
  for (int g = 0; g < 3; ++g) {
    const int s = g < count ? g : 0;       // (an absent problem: no tiles, the pointers of problem 0)
    ga.x[g] = reinterpret_cast<const f16*>(xs[s]);
    ga.q[g] = reinterpret_cast<const uint16_t*>(qidxs[s]);
    ga.y[g] = reinterpret_cast<f16*>(ys[s]);
    ga.n[g] = ns[s];
    ga.tile0[g + 1] = ga.tile0[g] + (g < count ? (ns[g] + cols - 1) / cols : 0);   // (n <= 2^31 - 1: below 2^26 tiles each)
  }
  ga.M = m;
  ga.K = k;
  ga.grid = reinterpret_cast<const uint64_t*>(a.grid);
  ga.grid2 = reinterpret_cast<const uint32_t*>(a.grid2);
  ga.resid_scale = a.scale;
  const int tiles = ga.tile0[3], cus = device_cu_count();
  auto go = [&](auto kern) -> int {
    return launch<decltype(kern)::value>(dim3(tiles < cus ? tiles : cus), dim3(1024), kSLds, stream, ga);
  };
  if (cb == kE8PRVQ4) {
    if (m <= 16) return one ? go(kernel_c<e8p_skinny_group_kernel<1, 16, 1>>) : go(kernel_c<e8p_skinny_group_kernel<2, 16, 1>>);
    return one ? go(kernel_c<e8p_skinny_group_kernel<1, 32, 1>>) : go(kernel_c<e8p_skinny_group_kernel<2, 32, 1>>);
  }
  if (cb == kD4) {
    if (m <= 16) return one ? go(kernel_c<e8p_skinny_group_kernel<1, 16, 2>>) : go(kernel_c<e8p_skinny_group_kernel<2, 16, 2>>);
    return one ? go(kernel_c<e8p_skinny_group_kernel<1, 32, 2>>) : go(kernel_c<e8p_skinny_group_kernel<2, 32, 2>>);
  }
  if (cb == kE8PRVQ3) {
    if (m <= 16) return one ? go(kernel_c<e8p_skinny_group_kernel<1, 16, 4>>) : go(kernel_c<e8p_skinny_group_kernel<2, 16, 4>>);
    return one ? go(kernel_c<e8p_skinny_group_kernel<1, 32, 4>>) : go(kernel_c<e8p_skinny_group_kernel<2, 32, 4>>);
  }
  if (cb == kHI) {
    if (m <= 16) return one ? go(kernel_c<e8p_skinny_group_kernel<1, 16, 3>>) : go(kernel_c<e8p_skinny_group_kernel<2, 16, 3>>);
    return one ? go(kernel_c<e8p_skinny_group_kernel<1, 32, 3>>) : go(kernel_c<e8p_skinny_group_kernel<2, 32, 3>>);
  }
  if (m <= 16) return one ? go(kernel_c<e8p_skinny_group_kernel<1, 16, 0>>) : go(kernel_c<e8p_skinny_group_kernel<2, 16, 0>>);
  return one ? go(kernel_c<e8p_skinny_group_kernel<1, 32, 0>>) : go(kernel_c<e8p_skinny_group_kernel<2, 32, 0>>);
}

}  // namespace quip
