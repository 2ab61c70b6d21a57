// The quantiser's incoherence transforms of H and W: fp32 / fp64 rows of n = K L elements, 64 <= L a power of two,
//     Y[r, :out_cols] = s_out * ( pad_n(s_in * X[r]) (Hk (x) H_L)^T f )[:out_cols],        f = scale / sqrt(L),
// quant.matmul_hadU on the (K, L) view of a row, in one launch; with store_t the result goes out transposed, (out_cols, rows)
// row major, so that a two-sided transform  U (S H S) U^T  is two launches and nothing else.
//
// Work split.  A workgroup of 512 lanes owns R consecutive rows and holds them in registers for the whole kernel: lane t has
// the 16-byte pieces (V = 4 fp32 | 2 fp64 elements) at flat index i = (c 512 + t) V of chunk c < CH = ceil(n / 512 V), rounded
// up to a power of two, of every row of its tile -- R CH V values, R = min(8, 32 / CH), at most 128 dwords.  X is read once,
// Y written once, nothing is re-read from memory.  Rows past `rows` and columns past in_cols are zeros.
//
// The transform.  L is a power of two and divides n, so the Walsh-Hadamard butterflies of all K segments of a row are the
// butterflies on the low log2 L bits of the flat index, whatever K is.  In this fixed order:
//   bits inside a piece:    in the lane's registers;
//   the 6 lane bits:        __shfl_xor, no LDS;
//   the 3 wave bits:        one LDS exchange per 8 / R chunks -- every lane writes its piece at its own place and reads the
//                           pieces of the 8 waves at its lane position, consecutive lanes consecutive 16 bytes both ways (no
//                           bank conflict), and folds them by the 3-level tree of its own output: the same sums and
//                           differences in the same order as the butterflies;
//   the chunk bits:         in the lane's registers again.
// Stages at and above bit log2 L are skipped.  A row's bits depend on that row alone.
//
// The K-mix, out[k', l] = sum_k Hk[k', k] y[k, l]: the values of one l lie L apart, in other lanes.  The row tile passes
// through the same 64 KB of LDS in slabs of W columns of l (all K segments and all R rows of a slab at once, W the largest
// power of two that fits): the owners of a slab write their pieces to [(r K + k) W + l], a barrier, then every owner sums its
// own output over k = 0 .. K - 1 by FMA in T against Hk from LDS (fp32 there, 16 KB at the most, widened at use; stored
// transposed already when hadK_t asks), consecutive lanes reading consecutive pieces.  K = 1 skips all of this.
//
// Stores.  s_in on load; s_out[j] f on store.  Plain: the 16-byte pieces along the row.  Transposed: a lane has the same j
// of all R rows and stores them as one run of R elements of output row j (16-byte pieces; 8 bytes for R = 2 in fp32), when
// rows % R == 0; element by element otherwise.  Row tiles that are neighbours in memory are mapped to workgroups 8 apart --
// the same XCD by the round-robin dispatch -- so that the partial lines of one output row meet in one L2 (`swizzle`).
// Vector loads / stores along the row need in_cols % V == 0 / out_cols % V == 0; other widths go element by element.
// Addresses are 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "launch.hip.h"

namespace quip {

namespace {

constexpr int kHwThreads = 512;
constexpr int kHwWaves = kHwThreads / 64;
constexpr int kHwExchangeBytes = 64 * 1024;                      // wave exchange: 8 (row, chunk) images of 8 KB; K-mix slabs
constexpr int kHwMaxK = 64;
constexpr int kHwLdsBytes = kHwExchangeBytes + kHwMaxK * kHwMaxK * (int)sizeof(float);
constexpr int kHwXcds = 8;

struct HadWideArgs {
  void* y;
  const void* x;
  const float* hadK;
  const void* s_in;
  const void* s_out;
  int64_t rows;
  double f;                 // scale / sqrt(L)
  unsigned tiles, per_xcd;  // row tiles; per_xcd > 0: blockIdx b serves tile (b % 8) per_xcd + b / 8
  int in_cols, out_cols, n, K, logL, logW, hadK_t, store_t;
};

template <typename T, int P>
struct Pack { typedef T type __attribute__((ext_vector_type(P))); };

template <typename T>
__device__ __forceinline__ T bfly_lane(T own, int mask, bool upper) {
  const T other = __shfl_xor(own, mask);
  return upper ? other - own : own + other;
}

template <typename T, int CH, int R>
__global__ __launch_bounds__(kHwThreads) void had_wide_rows_kernel(HadWideArgs a) {
  constexpr int V = 16 / (int)sizeof(T);
  constexpr int kChunk = kHwThreads * V;                         // elements of a row per chunk
  constexpr int kBatch = 8 / R;                                  // chunks per wave exchange
  constexpr int kLogCH = CH == 1 ? 0 : CH == 2 ? 1 : CH == 4 ? 2 : CH == 8 ? 3 : CH == 16 ? 4 : 5;
  static_assert(R * CH <= 32 && kBatch >= 1 && CH % kBatch == 0, "the tile is at most 128 dwords per lane");
  using VecT = typename Pack<T, V>::type;
  extern __shared__ __align__(16) unsigned char had_wide_lds[];
  T* ex = reinterpret_cast<T*>(had_wide_lds);
  float* hk = reinterpret_cast<float*>(had_wide_lds + kHwExchangeBytes);

  unsigned tile = blockIdx.x;
  if (a.per_xcd) tile = (blockIdx.x % kHwXcds) * a.per_xcd + blockIdx.x / kHwXcds;
  if (tile >= a.tiles) return;                                   // uniform, before any barrier
  const int64_t row0 = (int64_t)tile * R;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, K = a.K, L = 1 << a.logL;
  const int nch = (n + kChunk - 1) / kChunk;
  const T* X = reinterpret_cast<const T*>(a.x);
  T* Y = reinterpret_cast<T*>(a.y);

  if (K > 1)                                                     // read after the K-mix's first barriers
    for (int i = tid; i < K * K; i += kHwThreads) hk[i] = a.hadK_t ? a.hadK[(i % K) * K + i / K] : a.hadK[i];

  // ---- load, s_in ----
  T v[R][CH][V];
  {
    const T* s_in = reinterpret_cast<const T*>(a.s_in);
    const bool vec = a.in_cols % V == 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      int tv = tid;
      if constexpr (CH >= 16) asm volatile("" : "+v"(tv));         // as in the K-mix below
      const int i0 = (c * kHwThreads + tv) * V;
      T si[V];
#pragma unroll
      for (int e = 0; e < V; ++e) si[e] = (s_in && i0 + e < a.in_cols) ? s_in[i0 + e] : (T)1;
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int e = 0; e < V; ++e) v[r][c][e] = (T)0;
        if (row0 + r < a.rows && i0 < a.in_cols) {
          const T* p = X + (row0 + r) * (int64_t)a.in_cols + i0;
          if (vec) {
            const VecT q = *reinterpret_cast<const VecT*>(p);
#pragma unroll
            for (int e = 0; e < V; ++e) v[r][c][e] = q[e] * si[e];
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
              if (i0 + e < a.in_cols) v[r][c][e] = p[e] * si[e];
          }
        }
      }
    }
  }

  // ---- butterflies inside a piece ----
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      T* q = v[r][c];
      if constexpr (V == 4) {
        const T a0 = q[0] + q[1], a1 = q[0] - q[1], a2 = q[2] + q[3], a3 = q[2] - q[3];
        q[0] = a0 + a2;
        q[1] = a1 + a3;
        q[2] = a0 - a2;
        q[3] = a1 - a3;
      } else {
        const T a0 = q[0] + q[1], a1 = q[0] - q[1];
        q[0] = a0;
        q[1] = a1;
      }
    }
  }

  // ---- across the lanes of a wave ----
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    if ((V << b) >= L) continue;
    const bool upper = (lane >> b) & 1;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (c >= nch) continue;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < V; ++e) v[r][c][e] = bfly_lane(v[r][c][e], 1 << b, upper);
    }
  }

  // ---- across the waves: one exchange per kBatch chunks ----
  if (L > 64 * V) {
    const bool on0 = 64 * V < L, on1 = 128 * V < L, on2 = 256 * V < L;
    const bool u0 = wave & 1, u1 = wave & 2, u2 = wave & 4;
#pragma unroll
    for (int cb = 0; cb < CH; cb += kBatch) {
      if (cb >= nch) continue;                                     // uniform
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kBatch; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          VecT q;
#pragma unroll
          for (int e = 0; e < V; ++e) q[e] = v[r][cb + s][e];
          *reinterpret_cast<VecT*>(ex + (s * R + r) * kChunk + tid * V) = q;
        }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < kBatch; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          VecT t[8];
#pragma unroll
          for (int w = 0; w < 8; ++w)
            t[w] = *reinterpret_cast<const VecT*>(ex + (s * R + r) * kChunk + (w * 64 + lane) * V);
#pragma unroll
          for (int p = 0; p < 4; ++p)
            t[p] = on0 ? (u0 ? t[2 * p] - t[2 * p + 1] : t[2 * p] + t[2 * p + 1]) : (u0 ? t[2 * p + 1] : t[2 * p]);
#pragma unroll
          for (int p = 0; p < 2; ++p)
            t[p] = on1 ? (u1 ? t[2 * p] - t[2 * p + 1] : t[2 * p] + t[2 * p + 1]) : (u1 ? t[2 * p + 1] : t[2 * p]);
          t[0] = on2 ? (u2 ? t[0] - t[1] : t[0] + t[1]) : (u2 ? t[1] : t[0]);
#pragma unroll
          for (int e = 0; e < V; ++e) v[r][cb + s][e] = t[0][e];
        }
    }
  }

  // ---- across the chunks ----
#pragma unroll
  for (int b = 0; b < kLogCH; ++b) {
    if ((kChunk << b) >= L) continue;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (c & (1 << b)) continue;
      const int c2 = c | (1 << b);
      if (c2 >= nch) continue;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const T lo = v[r][c][e], hi = v[r][c2][e];
          v[r][c][e] = lo + hi;
          v[r][c2][e] = lo - hi;
        }
    }
  }

  // ---- the K-mix, slab by slab through LDS ----
  if (K > 1) {
    const int W = 1 << a.logW, slabs = L >> a.logW;
    for (int sl = 0; sl < slabs; ++sl) {
      int tv = tid;                                                // opaque per slab: the CH chunks' indices are recomputed
      asm volatile("" : "+v"(tv));                                 // where they are used, not kept live across the loop
      __syncthreads();
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int i0 = (c * kHwThreads + tv) * V, l = i0 & (L - 1), k = i0 >> a.logL;
        if (i0 < n && (l >> a.logW) == sl) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            VecT q;
#pragma unroll
            for (int e = 0; e < V; ++e) q[e] = v[r][c][e];
            *reinterpret_cast<VecT*>(ex + (r * K + k) * W + (l & (W - 1))) = q;
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int i0 = (c * kHwThreads + tv) * V, l = i0 & (L - 1), k = i0 >> a.logL;
        if (i0 < n && (l >> a.logW) == sl) {
          VecT acc[R];
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[r][e] = (T)0;
          const float* hrow = hk + k * K;
          const T* col = ex + (l & (W - 1));
          for (int kk = 0; kk < K; ++kk) {
            const T cf = (T)hrow[kk];
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const VecT q = *reinterpret_cast<const VecT*>(col + (r * K + kk) * W);
#pragma unroll
              for (int e = 0; e < V; ++e) acc[r][e] = __builtin_fma(cf, q[e], acc[r][e]);
            }
          }
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int e = 0; e < V; ++e) v[r][c][e] = acc[r][e];
        }
      }
    }
  }

  // ---- s_out f, store ----
  const T* s_out = reinterpret_cast<const T*>(a.s_out);
  const T f = (T)a.f;
  const bool vec = a.out_cols % V == 0, runs = a.rows % R == 0;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    int tv = tid;
    if constexpr (CH >= 16) asm volatile("" : "+v"(tv));
    const int i0 = (c * kHwThreads + tv) * V;
    if (i0 >= a.out_cols) continue;
    T so[V];
#pragma unroll
    for (int e = 0; e < V; ++e) so[e] = (s_out && i0 + e < a.out_cols) ? s_out[i0 + e] * f : f;
    if (!a.store_t) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (row0 + r >= a.rows) continue;
        T* p = Y + (row0 + r) * (int64_t)a.out_cols + i0;
        if (vec) {
          VecT q;
#pragma unroll
          for (int e = 0; e < V; ++e) q[e] = v[r][c][e] * so[e];
          *reinterpret_cast<VecT*>(p) = q;
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (i0 + e < a.out_cols) p[e] = v[r][c][e] * so[e];
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (i0 + e >= a.out_cols) continue;
        T* p = Y + (int64_t)(i0 + e) * a.rows + row0;
        constexpr int P = R < V ? R : V;                          // elements per store of a run
        if constexpr (P > 1) {
          if (runs) {
            using RunT = typename Pack<T, P>::type;
#pragma unroll
            for (int r = 0; r < R; r += P) {
              RunT q;
#pragma unroll
              for (int u = 0; u < P; ++u) q[u] = v[r + u][c][e] * so[e];
              *reinterpret_cast<RunT*>(p + r) = q;
            }
            continue;
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (row0 + r < a.rows) p[r] = v[r][c][e] * so[e];
      }
    }
  }
}

int floor_log2(int64_t x) {
  int b = 0;
  while ((x >> (b + 1)) > 0) ++b;
  return b;
}

template <typename T, int CH>
int had_wide_go(HadWideArgs a, int swizzle, hipStream_t stream) {
  constexpr int R = (32 / CH) < 8 ? (32 / CH) : 8;
  const int64_t tiles = (a.rows + R - 1) / R, per = (tiles + kHwXcds - 1) / kHwXcds;
  if (per * kHwXcds > 0x7fffffff) return QUIP_ERR_UNSUPPORTED;
  a.tiles = (unsigned)tiles;
  a.per_xcd = swizzle ? (unsigned)per : 0u;
  int64_t w = kHwExchangeBytes / ((int64_t)R * a.K * (int64_t)sizeof(T));      // >= 16: R <= 8, K <= 64
  a.logW = floor_log2(w) < a.logL ? floor_log2(w) : a.logL;
  const unsigned grid = swizzle ? (unsigned)(per * kHwXcds) : (unsigned)tiles;
  return launch<had_wide_rows_kernel<T, CH, R>>(dim3(grid), dim3(kHwThreads), kHwLdsBytes, stream, a);
}

template <typename T>
int had_wide_pick(const HadWideArgs& a, int swizzle, hipStream_t stream) {
  constexpr int kChunk = kHwThreads * 16 / (int)sizeof(T);
  const int nch = (a.n + kChunk - 1) / kChunk;
  if (nch <= 1) return had_wide_go<T, 1>(a, swizzle, stream);
  if (nch <= 2) return had_wide_go<T, 2>(a, swizzle, stream);
  if (nch <= 4) return had_wide_go<T, 4>(a, swizzle, stream);
  if (nch <= 8) return had_wide_go<T, 8>(a, swizzle, stream);
  if (nch <= 16) return had_wide_go<T, 16>(a, swizzle, stream);
  if constexpr (sizeof(T) == 8) return had_wide_go<T, 32>(a, swizzle, stream);
  return QUIP_ERR_UNSUPPORTED;
}

}  // namespace

// Shapes first (BAD_SHAPE), then the range this kernel serves (UNSUPPORTED); pointers are capi.hip's business.
int had_wide_rows_check(int dtype, int64_t rows, int in_cols, int out_cols, int n, int K) {
  if (rows < 1 || K < 1 || n < 1 || n % K != 0) return QUIP_ERR_BAD_SHAPE;
  const int L = n / K;
  if ((L & (L - 1)) != 0 || in_cols < 1 || in_cols > n || out_cols < 1 || out_cols > n) return QUIP_ERR_BAD_SHAPE;
  if (dtype != QUIP_DTYPE_F32 && dtype != QUIP_DTYPE_F64) return QUIP_ERR_UNSUPPORTED;
  if (K > kHwMaxK || L < 64 || n > 32768) return QUIP_ERR_UNSUPPORTED;
  return QUIP_OK;
}

int had_wide_rows_launch(void* y, const void* x, int dtype, int64_t rows, int in_cols, int out_cols, int n, int K,
                         const float* hadK, int hadK_t, const void* s_in, const void* s_out, double scale, int store_t,
                         int swizzle, hipStream_t stream) {
  const int rc = had_wide_rows_check(dtype, rows, in_cols, out_cols, n, K);
  if (rc != QUIP_OK) return rc;
  HadWideArgs a{};
  a.y = y;
  a.x = x;
  a.hadK = hadK;
  a.s_in = s_in;
  a.s_out = s_out;
  a.rows = rows;
  a.in_cols = in_cols;
  a.out_cols = out_cols;
  a.n = n;
  a.K = K;
  a.logL = floor_log2(n / K);
  a.f = scale / std::sqrt((double)(n / K));
  a.hadK_t = hadK_t != 0;
  a.store_t = store_t != 0;
  return dtype == QUIP_DTYPE_F64 ? had_wide_pick<double>(a, swizzle, stream) : had_wide_pick<float>(a, swizzle, stream);
}

}  // namespace quip
