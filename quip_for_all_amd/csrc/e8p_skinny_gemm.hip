// Skinny E8P12 product for 2 <= M <= 32 activation rows in ONE pass over the codes, gfx950.
//
//   Y[m, n] = sum_k X[m, k] * W[n, k],   W = decode(Qidxs (N, K/8) int16),  fp16 x fp16 -> fp32 -> fp16
//
// Replaces the 1 < M < 32 use of tinygemm_m16n8k16_chunk_kernel<.., BLayout_E8, ..> (origin_order.cu:388-555;
// e8p12.py:147-150) with the reference's own arithmetic: fp16 activations, exact fp16 weights, fp32 accumulation on
// the matrix cores, one fp16 rounding of the result.
//
// Why a second skinny path next to rows mode (e8p_gemv_mfma.hip): rows mode keeps the GEMV's exact integer
// arithmetic (every row bit identical to its bs = 1 result) but carries at most 5 activation rows per pass -- a
// workgroup has to hold the digit planes of every row it multiplies, 3 K bytes each -- so M = 16 costs 4 passes and
// M = 31 seven.  Here the activations stay fp16, as in the reference: v_mfma_f32_32x32x16_f16 takes 32 activation rows
// at once, one E8P code per lane is a complete B fragment (8 consecutive-k weights of one column, decoded by two LDS
// table lookups + XOR + the 0x5c00 | (4w + 128) fp16 identity, as in e8p_prefill_gemm.hip), and the codes are
// streamed exactly once.  What is given up is bit identity with the bs = 1 path (fp32 accumulation instead of exact
// integers); a row's result is still independent of the batch it is in, and the exact rows-mode path stays selectable
// (QuantLinear.skinny_exact / QUIP_SKINNY_EXACT=1).
//
// Mapping: workgroup = 16 waves = CB column blocks of 32 x (16 / CB) slices of K (CB = 1 when the matrix has few
// columns: more workgroups and shorter dependent chains per wave).  A wave walks its K slice in units of 128 k =
// four granules of 32 k = two MFMAs each.
//   codes: one 16-byte load per lane and unit (lane (n, kb): the unit's 8-k blocks 8 kb .. 8 kb + 7 of column n),
//     then two v_permlane32_swap exchange code pairs between the kb halves so that in granule i MFMA t multiplies
//     block 4 i + 2 kb + t -- the MFMA's k index is relabelled, activations follow the same labelling;
//   activations: an MFMA A fragment is 32 rows x 32 bytes, i.e. 64 lanes reading 64 different rows/segments.  Read
//     straight from L2 that costs one vector-memory lane slot each (measured: time grew by 0.25 us per activation row
//     at 4096 x 4096, 7.4 us from M = 1 to M = 31, whatever the row stride).  So a granule is brought in ROW
//     CONTIGUOUS -- one global_load_lds_dwordx4 = 16 rows x 64 bytes, four lanes per row, no staging registers --
//     into a ring of three granules per wave, and the fragments are read back from LDS (ds_read_b128; the 16-byte
//     pieces of a row are stored in the order p ^ ((row >> 1) & 3), applied on the SOURCE side because the LDS image
//     of such a load is lane-linear: 8 consecutive rows then fall into 8 different bank groups).
//   Rows >= M are not fetched (the lanes re-read row M - 1); a launch for M <= 16 stages 16 rows.
// All vector-memory traffic of the loop is counted by hand (vmcnt retires in order): per unit the issue order is
// s(4u+3)' = [codes of unit u + 2, granule 4u + 3], granule 4u + 4, 4u + 5, 4u + 6, each right after the granule
// three earlier has been consumed; past the end of the slice the last unit / granule is requested again, which keeps
// the counts constant.  The K slices are added in a fixed order through LDS (every wave reduces a share of the
// tile), so the result does not depend on scheduling.
// Bound: LDS / L2 issue (codes N K / 4 bytes once from HBM; activations M K 2 bytes per 32 columns from L2).
//
// MODE 1 = E8P12RVQ4B (e8p12_rvq4.py:37-45; origin_order.cu:337-385): a code is 32 bits, main << 16 | residual, both E8P12
// codes; the weight is fma(s, w_resid, w_main) in packed fp16 -- ONE fp16 rounding per weight, exactly what
// decompress_e8prvq4_origorder writes (quip_device.hip.h: rvq_combine), so the product is x . W of the reference's dense W.
// Per lane and unit two 16-byte loads (eight 4-byte codes), four table lookups and four v_pk_fma_f16 per MFMA.
// MODE 4 = E8P12RVQ3B (e8p12_rvq3.py:81-129; origin_order.cu:287-335): 3-byte codes [residual index, E8P code]; two 12-byte
// loads per lane and unit, a shift and two v_perm_b32 turn them into the dwords (main << 16 | residual << 8) of MODE 1's
// data movement; the residual is one 4-byte lookup (eight int4 = 2 x value, the reference's packed E81B table) turned into
// fp16 by 0x4c00 | (n ^ 8) << 6 = 16 + (n ^ 8) and one exact fma (x 0.5, - 12), then fma(s, w_resid, w_main) as in MODE 1.
// (Table space: the sign table keeps 8 copies instead of 16, the 16 KB hold 16 copies of the residual table.)
// MODE 2 = D4 (d4.py:26-96; origin_order.cu BLayout_D4): two one-byte codes per 8 weights -- the data movement of MODE 0 --
// and the table holds the fp16 entries themselves: a B fragment is two 8-byte lookups, no arithmetic.
// MODE 3 = HI (hi.py:41-50; origin_order.cu:1028-1051): eight nibbles per 8 weights -- the data movement of MODE 1 --,
// w = nibble - 7.5 through the 0x4c00 | n << 6 = 16 + n identity and one packed subtraction; no table.
// The body of a column tile is e8p_skinny_tile.hip.h, shared with the grouped launch (e8p_skinny_group.hip).
#include "e8p_skinny_tile.hip.h"

namespace quip {

namespace {

template <int CB, int MP, int MODE = 0>
__global__ __launch_bounds__(1024) void e8p_skinny_gemm_kernel(const f16* __restrict__ X,
                                                               const uint16_t* __restrict__ Wc,
                                                               const uint64_t* __restrict__ grid,
                                                               f16* __restrict__ Y, int M, int N, int K, float resid_scale,
                                                               const uint32_t* __restrict__ grid2) {
  // more than 32 rows: grid.y walks over chunks of 32 rows (each workgroup streams its columns' codes again; the
  // chunks of one column block run side by side and share them in L2)
  X += (size_t)blockIdx.y * 32 * K;
  Y += (size_t)blockIdx.y * 32 * N;
  M = min(32, M - (int)blockIdx.y * 32);
  skinny_tiles<CB, MP, MODE, false>(X, Wc, grid, Y, M, N, K, resid_scale, grid2, (int)blockIdx.x * (32 * CB), nullptr);
}

}  // namespace

// the single launch's choice of the tile, a function of n alone (see skinny_gemm_launch)
bool skinny_group_one_block(int n) { return (n + 63) / 64 < 2 * device_cu_count() / 3; }

bool e8p_skinny_gemm_supported(int m, int n, int k) {
  return m >= 1 && m <= 32 * 65535 && n >= 2 && n % 2 == 0 && k >= 128 && k % 128 == 0;
}

// a.grid: the packed E8P table (E8P12*), the fp16 (256, 4) table (D4), none (HI); a.scale: the fp16 residual scale (E8P12RVQ*);
// a.grid2: the packed E81B table (E8P12RVQ3B).  The branches below name the kernel instantiations: their order is the
// order of the kernels in the device code
int skinny_gemm_launch(CodebookId cb, const void* x, const void* qidxs, const CodebookArgs& a, void* y, int m, int n, int k,
                       hipStream_t stream) {
  if (cb == kE8PRVQ3 && k % 32 != 0) return QUIP_ERR_UNSUPPORTED;      // rows of 3 k / 8 bytes, dword aligned
  if (!e8p_skinny_gemm_supported(m, n, k)) return QUIP_ERR_UNSUPPORTED;
  // few columns: one column block of 32 per workgroup and 16 slices of K (more workgroups, shorter chains per wave);
  // many columns: two column blocks x 8 slices
  // (a function of n alone: the K slicing fixes the order of the fp32 sums, and a row's result must not depend on
  //  how many rows the launch has)
  const bool one = skinny_group_one_block(n);
  auto go = [&](auto kern, int cols) -> int {
    return launch<decltype(kern)::value>(dim3((n + cols - 1) / cols, (m + 31) / 32), dim3(1024), kSLds, stream,
                                         reinterpret_cast<const f16*>(x), reinterpret_cast<const uint16_t*>(qidxs),
                                         reinterpret_cast<const uint64_t*>(a.grid), reinterpret_cast<f16*>(y), m, n, k,
                                         a.scale, reinterpret_cast<const uint32_t*>(a.grid2));
  };
  if (cb == kE8PRVQ4) {
    if (m <= 16) return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 16, 1>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 16, 1>>, 64);
    return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 32, 1>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 32, 1>>, 64);
  }
  if (cb == kD4) {
    if (m <= 16) return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 16, 2>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 16, 2>>, 64);
    return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 32, 2>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 32, 2>>, 64);
  }
  if (cb == kE8PRVQ3) {
    if (m <= 16) return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 16, 4>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 16, 4>>, 64);
    return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 32, 4>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 32, 4>>, 64);
  }
  if (cb == kHI) {
    if (m <= 16) return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 16, 3>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 16, 3>>, 64);
    return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 32, 3>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 32, 3>>, 64);
  }
  if (m <= 16) return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 16>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 16>>, 64);
  return one ? go(kernel_c<e8p_skinny_gemm_kernel<1, 32>>, 32) : go(kernel_c<e8p_skinny_gemm_kernel<2, 32>>, 64);
}

}  // namespace quip

