// The quantiser's Hessian accumulation as one symmetric rank-k update in fp64 on the matrix cores:
//     H  <- keep H  + s_h  X^T X          X (rows, n) row major, fp16 | bf16 | fp32;  H (n, n), mu (n) fp64
//     mu <- keep mu + s_mu colsum(X)
// fp16, bf16 and fp32 widen to fp64 exactly and a product of two fp32 values is exact in fp64, so this is the fp64 arithmetic
// of `x = X.double().t(); H = keep H + s_h x @ x.t()` without the fp64 copy of X, without the upper triangle's products and
// without the n x n temporary.
//
// Work split.  C = X^T X is cut into tiles of 128 x 128; one workgroup of 4 waves owns one tile pair (ti >= tj) of the lower
// triangle -- blockIdx.x counts them row by row, the kernel takes the integer square root -- and runs the whole loop over
// the rows of X in increasing order.  No split over rows, no atomics: an element of H has one owner and a fixed order of
// summation, so its bits depend on X, H and the scalars alone.  Wave w holds the 64 x 64 quarter (w >> 1, w & 1) as 4 x 4
// accumulators of v_mfma_f64_16x16x4_f64: 64 fp64 per lane.
//
// Data movement.  C[i, j] = sum_r X[r, i] X[r, j]: both operands of a tile are row segments of X, X[r0 : r0 + 32, i0 : i0 + 128]
// and the same at j0, contiguous along i.  A stage is kHessianKB = 32 rows.  The two panels of a stage (one on a diagonal
// tile, which multiplies it with itself) go global -> registers as 16-byte pieces, one stage ahead of the products, and from
// the registers into one of two LDS buffers in the INPUT dtype, image [k][i] with a pitch of 144 elements: lane (m = lane & 15,
// k = lane >> 4) of an MFMA reads element [4 kk + k][16 b + m], the four k of a wave 16 elements' banks apart, and widens it.
// One barrier per stage: a buffer is overwritten one stage after its last read.  Rows >= rows and columns >= n are zero in
// LDS (n % 8 == 0 and the pieces are 4 or 8 elements, so a piece is inside or outside as a whole); stores are masked.
// Addresses are 64-bit: rows * n and n * n pass 2^31.
//
// Epilogue.  The owner reads H_old[i, j] of its tile (the lower triangle; H is symmetric by this kernel's own doing), forms
// keep H_old + s_h acc and stores it to [i, j] and, off the diagonal tiles, the same register to [j, i]: H == H^T exactly.
// A diagonal tile computes and stores all 128 x 128 of itself; its [i, j] and [j, i] are the same sum in the same order.
// mu: the diagonal tile of columns [i0, i0 + 128) has that panel in LDS anyway.  Thread t sums column t & 127 over the rows
// 16 (t >> 7) .. + 16 of every stage in increasing order, the two halves are added at the end: a fixed order, no second
// pass over X.
#include <hip/hip_runtime.h>

#include "launch.hip.h"

namespace quip {

namespace {

constexpr int kHessianKB = QUIP_HESSIAN_ROW_BLOCK;      // rows of X per stage
constexpr int kTile = 128;                              // columns of X per panel: the tile is kTile x kTile
constexpr int kPitch = kTile + 16;                      // elements per LDS row: consecutive rows 16 elements' banks apart
static_assert(kHessianKB == 32, "two halves of 16 rows in the column sums, 8 MFMA steps per stage");

typedef double double4_t __attribute__((ext_vector_type(4)));

template <int kDtype>
struct Elem;
template <>
struct Elem<QUIP_DTYPE_F16> {
  using type = _Float16;
  static __device__ __forceinline__ double widen(type v) { return (double)(float)v; }
};
template <>
struct Elem<QUIP_DTYPE_BF16> {
  using type = uint16_t;
  static __device__ __forceinline__ double widen(type v) { return (double)__uint_as_float((uint32_t)v << 16); }
};
template <>
struct Elem<QUIP_DTYPE_F32> {
  using type = float;
  static __device__ __forceinline__ double widen(type v) { return (double)v; }
};

template <int kDtype>
constexpr int hessian_panel_bytes() { return kHessianKB * kPitch * (int)sizeof(typename Elem<kDtype>::type); }
template <int kDtype>
constexpr int hessian_lds_bytes() { return 4 * hessian_panel_bytes<kDtype>(); }      // two buffers of two panels

// row ti of the lower triangle holds tiles ti (ti + 1) / 2 .. + ti
__device__ __forceinline__ void tile_of(unsigned t, int& ti, int& tj) {
  int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (r * (r + 1) / 2 > (int64_t)t) --r;
  while ((r + 1) * (r + 2) / 2 <= (int64_t)t) ++r;
  ti = (int)r;
  tj = (int)((int64_t)t - r * (r + 1) / 2);
}

template <int kDtype>
__global__ __launch_bounds__(256, 2) void hessian_syrk_kernel(double* H, double* mu, const void* __restrict__ xv,
                                                              int64_t rows, int n, double keep, double s_h, double s_mu) {
  using T = typename Elem<kDtype>::type;
  constexpr int kVec = 16 / (int)sizeof(T);                      // elements per 16-byte piece
  constexpr int kRowVecs = kTile / kVec;                         // pieces per panel row
  constexpr int kPieces = kHessianKB * kRowVecs / 256;           // pieces per thread and panel
  constexpr int kPanel = kHessianKB * kPitch;                    // elements per panel image
  extern __shared__ __align__(16) unsigned char hessian_lds[];
  T* lds = reinterpret_cast<T*>(hessian_lds);
  const T* X = reinterpret_cast<const T*>(xv);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, q = lane >> 4, wi = wave >> 1, wj = wave & 1;
  int ti, tj;
  tile_of(blockIdx.x, ti, tj);
  const bool diag = ti == tj;
  const int i0 = ti * kTile, j0 = tj * kTile;
  const int panels = diag ? 1 : 2;

  uint4 pre[2][kPieces];
  auto load_stage = [&](int64_t r0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (p >= panels) break;
      const int c0 = p == 0 ? i0 : j0;
#pragma unroll
      for (int s = 0; s < kPieces; ++s) {
        const int u = tid + s * 256, row = u / kRowVecs, col = c0 + (u % kRowVecs) * kVec;
        pre[p][s] = make_uint4(0u, 0u, 0u, 0u);
        if (r0 + row < rows && col < n) pre[p][s] = *reinterpret_cast<const uint4*>(X + (r0 + row) * (int64_t)n + col);
      }
    }
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (p >= panels) break;
#pragma unroll
      for (int s = 0; s < kPieces; ++s) {
        const int u = tid + s * 256, row = u / kRowVecs, col = (u % kRowVecs) * kVec;
        *reinterpret_cast<uint4*>(lds + (buf * 2 + p) * kPanel + row * kPitch + col) = pre[p][s];
      }
    }
  };

  double4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = double4_t{0.0, 0.0, 0.0, 0.0};
  double colsum = 0.0;

  const int64_t stages = (rows + kHessianKB - 1) / kHessianKB;
  load_stage(0);
  store_stage(0);
  __syncthreads();
  for (int64_t st = 0; st < stages; ++st) {
    const int buf = (int)(st & 1);
    const bool more = st + 1 < stages;
    if (more) load_stage((st + 1) * kHessianKB);
    const T* pi = lds + (buf * 2) * kPanel;
    const T* pj = diag ? pi : pi + kPanel;
    const T* pa = pi + q * kPitch + wi * 64 + m;
    const T* pb = pj + q * kPitch + wj * 64 + m;
#pragma unroll
    for (int kk = 0; kk < kHessianKB / 4; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = Elem<kDtype>::widen(pa[kk * 4 * kPitch + e * 16]);
        b[e] = Elem<kDtype>::widen(pb[kk * 4 * kPitch + e * 16]);
      }
#pragma unroll
      for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
          acc[ib][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ib], b[jb], acc[ib][jb], 0, 0, 0);
    }
    if (diag) {
      const T* pc = pi + (tid >> 7) * 16 * kPitch + (tid & 127);
#pragma unroll
      for (int k = 0; k < 16; ++k) colsum += Elem<kDtype>::widen(pc[k * kPitch]);
    }
    if (more) store_stage(buf ^ 1);
    __syncthreads();
  }

  // accumulator element v of lane (m, q) in block (ib, jb): C[16 ib + 4 v + q][16 jb + m]
#pragma unroll
  for (int ib = 0; ib < 4; ++ib) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = i0 + wi * 64 + ib * 16 + 4 * v + q;
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const int j = j0 + wj * 64 + jb * 16 + m;
        if (i < n && j < n) {
          const int64_t at = (int64_t)i * n + j;
          const double h = keep * H[at] + s_h * acc[ib][jb][v];
          H[at] = h;
          if (!diag) H[(int64_t)j * n + i] = h;
        }
      }
    }
  }
  if (diag) {      // uniform over the workgroup; the loop's last barrier has passed, the panels are dead
    double* half = reinterpret_cast<double*>(hessian_lds);
    if (tid >= kTile) half[tid - kTile] = colsum;
    __syncthreads();
    const int c = i0 + tid;
    if (tid < kTile && c < n) mu[c] = keep * mu[c] + s_mu * (colsum + half[tid]);
  }
}

}  // namespace

int hessian_row_block() { return kHessianKB; }

// n >= 8, n % 8 == 0, rows >= 1, dtype one of QUIP_DTYPE_*: BAD_SHAPE / UNSUPPORTED otherwise; pointers are capi.hip's business
int hessian_accumulate_launch(void* H, void* mu, const void* x, int dtype, int64_t rows, int n, double keep, double s_h,
                              double s_mu, hipStream_t stream) {
  if (n < 8 || n % 8 != 0 || rows < 1) return QUIP_ERR_BAD_SHAPE;
  if (dtype != QUIP_DTYPE_F16 && dtype != QUIP_DTYPE_BF16 && dtype != QUIP_DTYPE_F32) return QUIP_ERR_UNSUPPORTED;
  const int64_t t = (n + kTile - 1) / kTile, tiles = t * (t + 1) / 2;
  if (tiles > 0x7fffffff) return QUIP_ERR_UNSUPPORTED;
  auto go = [&](auto k, int lds) {
    return launch<decltype(k)::value>(dim3((unsigned)tiles), dim3(256), lds, stream, reinterpret_cast<double*>(H),
                                      reinterpret_cast<double*>(mu), x, rows, n, keep, s_h, s_mu);
  };
  if (dtype == QUIP_DTYPE_F16) return go(kernel_c<hessian_syrk_kernel<QUIP_DTYPE_F16>>, hessian_lds_bytes<QUIP_DTYPE_F16>());
  if (dtype == QUIP_DTYPE_BF16) return go(kernel_c<hessian_syrk_kernel<QUIP_DTYPE_BF16>>, hessian_lds_bytes<QUIP_DTYPE_BF16>());
  return go(kernel_c<hessian_syrk_kernel<QUIP_DTYPE_F32>>, hessian_lds_bytes<QUIP_DTYPE_F32>());
}

}  // namespace quip
