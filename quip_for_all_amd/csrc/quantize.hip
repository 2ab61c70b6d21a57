// Quantise-time nearest-codeword search in the E8P12 codebook.
//
// Replaces E8P12_codebook.round / quantize (e8p12.py:125-137; also the first stage of
// e8p12_rvq3.py:81-92 and both stages of e8p12_rvq4.py:32-45):
//     idx = argmax_c ( 2 x . g_c - |g_c|^2 )  over the 65 536 codewords,   vals = g_idx
// which the reference evaluates as a dense (N, 8) x (8, 65 536) GEMM per LDLQ step (quant.py:103-135).
//
// The codebook is structured (origin_order.cu:211-253 read backwards): with b_e the abs-table row
// (eight half-integers, column 7 negative when the row's sum is odd, e8p12.py:72-78),
//     g = D b_e + s 1,   D = diag(+-1) with an EVEN number of -1,   s = +1/4 (par = 0) or -1/4 (par = 1),
//     code = e << 8 | (sv ^ par),  bit (7 - [0,2,1,3,4,6,5,7][j]) of sv <=> D_j = -1.
// For fixed (e, s), with y = x - s 1:
//     2 x.g - |g|^2 = 2 sum_j D_j b_j y_j + 2 s sum_j x_j - |b_e|^2 - 8 s^2
// is maximised by D_j = sign(b_j y_j); if that takes an odd number of -1 the cheapest repair flips the
// column with the smallest |b_j y_j|.  So the exact arg max needs 2 x 256 candidates of ~25 operations
// instead of 65 536 dot products: kLanes = 8 lanes per vector, each scanning 32 table rows (table in LDS),
// then an 8-lane shuffle arg max -- ~14 K operations per vector, and an LDLQ step (N = out_features vectors,
// issued thousands of times in sequence) has the latency of 64 candidates, not of a GEMM.
//
// Ties (a measure-zero set: some b_j y_j == 0, or two candidates with equal score) resolve to the
// lowest (e, par, column) in scan order, which need not be the lowest code: among candidates of equal score
// the lowest e wins, then par = 0 before par = 1; y_j == 0 counts as positive; an odd flip count is repaired
// on the first (lowest-index) column among those with the smallest b_j |y_j|.  Every instantiation of the
// scan and all three panel templates follow this one rule (tests/test_gpu_quantize_hard_cases.py holds them
// to it by equality on targets that are multiples of 1/8, where no fp32 rounding takes part).  Near-ties inside
// fp32 rounding of the score may resolve differently from a GEMM-based arg max.  Either way the returned point
// is a nearest codeword to within that rounding (tests/test_gpu_quantize.py states the bound;
// tests/quantize_hard_cases.py derives one from the scan's operations).
//
// Second kernel, further down: ldlq_panel_kernel runs the LDLQ recursion over a whole panel of <= 128 columns in one
// launch, with this search in place at every column group (the scan and the winner's reconstruction are device
// functions that both kernels call).  The kernel is a template over the rounding step of a group: E8P12 (one search), or the
// two residual codebooks E8P12RVQ4B / E8P12RVQ3B (a second search on the scaled residual of the first, same launch).
#include <hip/hip_runtime.h>

#include "quip_device.hip.h"
#include "launch.hip.h"

namespace quip {

namespace {

// ---- the search as device functions: e8p_quantize_kernel and ldlq_panel_kernel run the same instructions on the same
// fp32 target, so both choose the same codeword ------------------------------------------------------------------------

// thread e of 256 builds abs-table row e: |b_e| in natural column order, |b_e|^2, and whether column 7 is negative
__device__ __forceinline__ void e8p_table_row(int e, const uint64_t* __restrict__ grid_packed_abs, float (*tb)[8],
                                              float* tn, int* tneg) {
  const uint64_t p = grid_packed_abs[e];
  float n2 = 0.f;
  int neg = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    // byte j of the packed entry = 4 * value of column [0,2,1,3,4,6,5,7][j] (self-inverse permutation)
    const int col = e8p_byte_of_pos(j);
    const int v4 = (int)(int8_t)((p >> (8 * j)) & 0xff);
    const float v = 0.25f * (float)v4;
    tb[e][col] = fabsf(v);
    if (col == 7 && v4 < 0) neg = 1;
    n2 += v * v;
  }
  tn[e] = n2;
  tneg[e] = neg;
}

// candidate scan: lane `sub` of the vector's kLanes lanes scans 256 / kLanes table rows x 2 shifts, then the lanes
// agree on the arg max.  Returns best_e * 2 + best_par on every lane.  All kLanes lanes must call it.
template <int kLanes>
__device__ __forceinline__ int e8p_scan(const float (&xv)[8], int sub, const float (*tb)[8], const float* tn,
                                        const int* tneg) {
  float ay[2][8];     // |x_j - s| for s = +1/4, -1/4
  int ypar[2];        // parity of the number of negative (x_j - s)
  float cs[2];        // 2 s sum x - 8 s^2
  float sx = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) sx += xv[j];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float s = p ? -0.25f : 0.25f;
    int par = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float y = xv[j] - s;
      ay[p][j] = fabsf(y);
      par ^= (y < 0.f) ? 1 : 0;
    }
    ypar[p] = par;
    cs[p] = 2.f * s * sx - 0.5f;
  }
  float best = -3.0e38f;
  int best_e = 0, best_p = 0;
  for (int e = sub * (256 / kLanes); e < (sub + 1) * (256 / kLanes); ++e) {
    float b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = tb[e][j];
    const float n2 = tn[e];
    const int neg = tneg[e];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float sum = 0.f, mn = 3.0e38f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = b[j] * ay[p][j];
        sum += t;
        mn = fminf(mn, t);
      }
      // number of -1 in D relative to b_e (whose column 7 may itself be negative): negatives of y, plus one
      // if b_7 < 0; odd -> give up the cheapest column
      const int odd = ypar[p] ^ neg;
      const float score = 2.f * (sum - (odd ? 2.f * mn : 0.f)) + cs[p] - n2;
      if (score > best) { best = score; best_e = e; best_p = p; }
    }
  }
  // arg max over the vector's kLanes lanes: higher score, then the earlier (e, par) like a sequential scan
  int key = best_e * 2 + best_p;
#pragma unroll
  for (int off = 1; off < kLanes; off <<= 1) {
    const float os = __shfl_xor(best, off, 64);
    const int ok = __shfl_xor(key, off, 64);
    if (os > best || (os == best && ok < key)) { best = os; key = ok; }
  }
  return key;
}

// rebuild the winner of e8p_scan: signs, the repaired column, the values; returns the code
__device__ __forceinline__ int e8p_rebuild(const float (&xv)[8], int key, const float (*tb)[8], const int* tneg,
                                           float (&out)[8]) {
  const int best_e = key >> 1, best_p = key & 1;
  const float s = best_p ? -0.25f : 0.25f;
  float b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = tb[best_e][j];
  const int neg7 = tneg[best_e];
  int flip[8];     // D_j == -1 relative to the SIGNED b_e
  float mn = 3.0e38f;
  int jm = 0, cnt = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float y = xv[j] - s;
    const int want_neg = y < 0.f ? 1 : 0;                 // sign of the codeword's (g_j - s)
    const int base_neg = (j == 7 && neg7) ? 1 : 0;        // sign of b_e's column
    flip[j] = want_neg ^ base_neg;
    cnt += flip[j];
    const float t = b[j] * fabsf(y);
    if (t < mn) { mn = t; jm = j; }
  }
  if (cnt & 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j == jm) flip[j] ^= 1;
  }
  int sv = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sv |= flip[j] << (7 - e8p_byte_of_pos(j));   // the sign bit of column j is the one of its packed byte
    const float signed_b = ((j == 7 && neg7) ? -b[j] : b[j]);
    out[j] = (flip[j] ? -signed_b : signed_b) + s;
  }
  return (best_e << 8) | (sv ^ best_p);
}

template <int kLanes>
__global__ __launch_bounds__(256) void e8p_quantize_kernel(const float* __restrict__ x, int64_t nvec,
                                                          const uint64_t* __restrict__ grid_packed_abs,
                                                          float* __restrict__ vals, int64_t* __restrict__ idx) {
  __shared__ float tb[256][8];    // |b_e|, natural column order
  __shared__ float tn[256];       // |b_e|^2
  __shared__ int tneg[256];       // column 7 of b_e is negative
  e8p_table_row(threadIdx.x, grid_packed_abs, tb, tn, tneg);
  __syncthreads();
  const int sub = threadIdx.x & (kLanes - 1);
  int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kLanes;
  const bool valid = i < nvec;
  i = valid ? i : nvec - 1;     // keep every lane in the shuffles below
  float xv[8];
  {
    const float4 a = reinterpret_cast<const float4*>(x + i * 8)[0];
    const float4 b = reinterpret_cast<const float4*>(x + i * 8)[1];
    xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w; xv[4] = b.x; xv[5] = b.y; xv[6] = b.z; xv[7] = b.w;
  }
  const int key = e8p_scan<kLanes>(xv, sub, tb, tn, tneg);
  if (!valid || sub != 0) return;
  float out[8];
  const int code = e8p_rebuild(xv, key, tb, tneg, out);
  idx[i] = (int64_t)code;
  reinterpret_cast<float4*>(vals + i * 8)[0] = make_float4(out[0], out[1], out[2], out[3]);
  reinterpret_cast<float4*>(vals + i * 8)[1] = make_float4(out[4], out[5], out[6], out[7]);
}

// ---- the second stage of the residual codebooks (e8p12_rvq4.py:37-45, e8p12_rvq3.py:81-92) ----------------------------------
//     r = (t - a) / s,   b = Q2(r),   hat = a + b * s
// with every operation rounded to fp32 on its own: the stepwise route and the decoders form hat by a multiplication and
// an addition, so neither may contract into an FMA, and the division is the IEEE one (not a reciprocal).
__device__ __forceinline__ float rvq_residual(float t, float a, float s) {
#pragma clang fp contract(off)
  return (t - a) / s;
}
__device__ __forceinline__ float rvq_combine(float a, float b, float s) {
#pragma clang fp contract(off)
  const float bs = b * s;
  return a + bs;
}

// E81B (256 entries) in LDS: entry e at slot (e % 32) * 8 + e / 32, so that the 8 lanes of a row, which scan entries
// sub * 32 + i at the same i, read 64 consecutive floats (no bank conflict) instead of 8 addresses 1 KB apart.
__device__ __forceinline__ int e81b_slot(int e) { return (e & 31) * 8 + (e >> 5); }

// thread e of 256 loads entry e and its squared norm (entries are multiples of 1/2: the norm is exact in any order)
__device__ __forceinline__ void e81b_table_row(int e, const float* __restrict__ resid_grid, float (*eb)[8], float* en) {
  const float4 lo = reinterpret_cast<const float4*>(resid_grid + e * 8)[0];
  const float4 hi = reinterpret_cast<const float4*>(resid_grid + e * 8)[1];
  const float g[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const int slot = e81b_slot(e);
  float n2 = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    eb[slot][j] = g[j];
    n2 += g[j] * g[j];
  }
  en[slot] = n2;
}

// dense arg max_c 2 r . g_c - |g_c|^2 over the 256 entries: lane `sub` of the row's 8 lanes scans entries sub * 32 ..
// sub * 32 + 31 in increasing order, then the lanes agree.  The dot product is eight products summed left to right, each
// rounded to fp32 (no FMA: the score is then the one an elementwise fp32 evaluation gives, which the tests write out);
// equal scores resolve to the lowest index inside a lane (strict >) and across lanes.  Returns the index on every lane.
__device__ __forceinline__ int e81b_scan(const float (&rv)[8], int sub, const float (*eb)[8], const float* en) {
#pragma clang fp contract(off)
  float best = -3.0e38f;
  int key = sub * 32;
  for (int i = 0; i < 32; ++i) {
    const int slot = i * 8 + sub;
    float dot = rv[0] * eb[slot][0];
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      const float pj = rv[j] * eb[slot][j];
      dot = dot + pj;
    }
    const float score = 2.f * dot - en[slot];      // 2 * dot is exact: one rounding
    if (score > best) { best = score; key = sub * 32 + i; }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) {
    const float os = __shfl_xor(best, off, 64);
    const int ok = __shfl_xor(key, off, 64);
    if (os > best || (os == best && ok < key)) { best = os; key = ok; }
  }
  return key;
}

// ---- one LDLQ panel in one launch ---------------------------------------------------------------------------
// For each of m rows independently, over the c / 8 column groups of the panel from the right:
//     target_k = A_k + ( B_k + sum_{j > k} (A_j - hat_j) M[j, k] ) P_k,   (hat_k, idx_k) = nearest codeword of target_k
// kPanelLanes = 8 lanes per row (the search's split), 32 rows per workgroup of 256.  Lane `sub` of a row owns column
// lo + sub of the current group: it sums that column's feedback over the row's running differences E_j = A_j - hat_j in
// increasing j by fp32 FMA (a fixed order: a row's bits depend on that row alone), the eight lanes exchange the target by
// shuffles, search together, and each stores its own column of hat and of E.
// LDS (dynamic): the abs table | M (c, c) | P (c / 8, 8, 8) | E as [column][row of the workgroup] (the 8 rows of a wave on 8
// banks, the row's 8 lanes on one address) | for kStepRVQ3 the E81B entries and norms.  E of a row is written and read by that
// row's 8 lanes only; the barrier per group orders the LDS store before the next group's loads.
// kStep is the rounding of one group's fp32 target t (already on the row's 8 lanes):
//   kStepE8P   hat = a = nearest E8P12 codeword of t,                                   code = code_a
//   kStepRVQ4  r = (t - a) / s, b = nearest E8P12 codeword of r, hat = a + b * s,       code = code_a << 16 | code_b
//   kStepRVQ3  the same with b = the dense arg max over the 256 E81B entries,           code = code_a <<  8 | idx_b
// (s = resid_scale, a kernel argument).  kStepRVQ3 keeps the E81B table and its norms in LDS behind E (+9 KB).
constexpr int kPanelRows = 32;
constexpr int kPanelMaxCols = 128;
constexpr int kPanelTableFloats = 256 * 8 + 256 + 256;
constexpr int kResidTableFloats = 256 * 8 + 256;
constexpr int kStepE8P = 0, kStepRVQ4 = 1, kStepRVQ3 = 2;

__host__ __device__ constexpr int ldlq_panel_lds_bytes(int c, int step = kStepE8P) {
  return 4 * (kPanelTableFloats + c * c + 8 * c + kPanelRows * c + (step == kStepRVQ3 ? kResidTableFloats : 0));
}

template <int kStep>
__global__ __launch_bounds__(256) void ldlq_panel_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                        const float* __restrict__ M, const float* __restrict__ P,
                                                        int64_t m, int c, const uint64_t* __restrict__ grid_packed_abs,
                                                        const float* __restrict__ resid_grid, float resid_scale,
                                                        float* __restrict__ hat, int64_t* __restrict__ idx) {
  extern __shared__ float panel_lds[];
  float (*tb)[8] = reinterpret_cast<float (*)[8]>(panel_lds);
  float* tn = panel_lds + 256 * 8;
  int* tneg = reinterpret_cast<int*>(panel_lds + 256 * 8 + 256);
  float* Ms = panel_lds + kPanelTableFloats;
  float* Ps = Ms + c * c;
  float* Es = Ps + 8 * c;
  float (*eb)[8] = reinterpret_cast<float (*)[8]>(Es + kPanelRows * c);      // kStepRVQ3 only
  float* en = Es + kPanelRows * c + 256 * 8;
  e8p_table_row(threadIdx.x, grid_packed_abs, tb, tn, tneg);
  if constexpr (kStep == kStepRVQ3) e81b_table_row(threadIdx.x, resid_grid, eb, en);
  for (int i = threadIdx.x; i < c * c / 4; i += 256)      // c % 8 == 0, M 16-byte aligned
    reinterpret_cast<float4*>(Ms)[i] = reinterpret_cast<const float4*>(M)[i];
  if (P != nullptr)
    for (int i = threadIdx.x; i < 2 * c; i += 256)
      reinterpret_cast<float4*>(Ps)[i] = reinterpret_cast<const float4*>(P)[i];
  __syncthreads();
  const int sub = threadIdx.x & 7, r = threadIdx.x >> 3;
  int64_t row = (int64_t)blockIdx.x * kPanelRows + r;
  const bool valid = row < m;
  row = valid ? row : m - 1;      // rows past the end repeat the last row (they take part in shuffles and barriers) and store nothing
  const float* __restrict__ a = A + row * c;
  const float* __restrict__ b = B + row * c;
  const int groups = c / 8;
  float a_cur = a[c - 8 + sub], b_cur = b[c - 8 + sub];
  for (int k = groups - 1; k >= 0; --k) {
    const int lo = k * 8, hi = lo + 8;
    float a_nxt = 0.f, b_nxt = 0.f;
    if (k > 0) { a_nxt = a[lo - 8 + sub]; b_nxt = b[lo - 8 + sub]; }     // the next group's operands, behind this group's search
    float acc = 0.f;
#pragma unroll 8
    for (int j = hi; j < c; ++j) acc = fmaf(Es[j * kPanelRows + r], Ms[j * c + lo + sub], acc);
    const float t = b_cur + acc;
    float tgt;
    if (P != nullptr) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) s = fmaf(__shfl(t, q, 8), Ps[(lo + q) * 8 + sub], s);
      tgt = a_cur + s;
    } else {
      tgt = a_cur + t;
    }
    float xv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) xv[q] = __shfl(tgt, q, 8);
    const int key = e8p_scan<8>(xv, sub, tb, tn, tneg);
    float out[8];
    int64_t code = e8p_rebuild(xv, key, tb, tneg, out);
    if constexpr (kStep != kStepE8P) {
      float rv[8], res[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) rv[q] = rvq_residual(xv[q], out[q], resid_scale);
      if constexpr (kStep == kStepRVQ4) {
        const int key_b = e8p_scan<8>(rv, sub, tb, tn, tneg);
        code = (code << 16) | (int64_t)e8p_rebuild(rv, key_b, tb, tneg, res);
      } else {
        const int idx_b = e81b_scan(rv, sub, eb, en);
        const int slot = e81b_slot(idx_b);
#pragma unroll
        for (int q = 0; q < 8; ++q) res[q] = eb[slot][q];
        code = (code << 8) | (int64_t)idx_b;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) out[q] = rvq_combine(out[q], res[q], resid_scale);
    }
    float mine = out[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) mine = (sub == q) ? out[q] : mine;
    Es[(lo + sub) * kPanelRows + r] = a_cur - mine;
    if (valid) {
      hat[row * c + lo + sub] = mine;
      if (sub == 0) idx[row * groups + k] = code;
    }
    __syncthreads();
    a_cur = a_nxt;
    b_cur = b_nxt;
  }
}

}  // namespace

int e8p_quantize_launch(const void* x, int64_t nvec, const void* grid_packed_abs, void* vals, void* idx,
                        hipStream_t stream) {
  if (nvec <= 0) return QUIP_OK;
  const int threads = 256;   // == table rows: thread e builds row e
  // LDLQ steps (N = out_features, one after the other): 8 lanes per vector for latency; big batches: one
  // lane per vector for throughput (measured 262 144 vectors: 97 us vs 178 us; 4096: 43 vs 16 us)
  const int lanes = nvec < 65536 ? 8 : 1;
  const int64_t blocks = (nvec * lanes + threads - 1) / threads;
  if (blocks > 0x7fffffff) return QUIP_ERR_BAD_SHAPE;
  const dim3 grid((unsigned)blocks), block(threads);
  const float* xf = reinterpret_cast<const float*>(x);
  const uint64_t* tab = reinterpret_cast<const uint64_t*>(grid_packed_abs);
  float* v = reinterpret_cast<float*>(vals);
  int64_t* ix = reinterpret_cast<int64_t*>(idx);
  return lanes == 8 ? launch<e8p_quantize_kernel<8>>(grid, block, 0, stream, xf, nvec, tab, v, ix)
                    : launch<e8p_quantize_kernel<1>>(grid, block, 0, stream, xf, nvec, tab, v, ix);
}

int ldlq_panel_launch(const void* A, const void* B, const void* M, const void* P, int64_t m, int c,
                      const void* grid_packed_abs, void* hat, void* idx, hipStream_t stream) {
  if (m <= 0) return QUIP_OK;
  if (c < 8 || c % 8 != 0 || c > kPanelMaxCols) return QUIP_ERR_BAD_SHAPE;
  const int64_t blocks = (m + kPanelRows - 1) / kPanelRows;
  if (blocks > 0x7fffffff) return QUIP_ERR_BAD_SHAPE;
  return launch<ldlq_panel_kernel<kStepE8P>>(dim3((unsigned)blocks), dim3(256), ldlq_panel_lds_bytes(c), stream,
                                             reinterpret_cast<const float*>(A), reinterpret_cast<const float*>(B),
                                             reinterpret_cast<const float*>(M), reinterpret_cast<const float*>(P), m, c,
                                             reinterpret_cast<const uint64_t*>(grid_packed_abs),
                                             static_cast<const float*>(nullptr), 0.f, reinterpret_cast<float*>(hat),
                                             reinterpret_cast<int64_t*>(idx));
}

// resid_grid == nullptr: the E8P12RVQ4B step; else (256, 8) fp32 E81B entries: the E8P12RVQ3B step
int ldlq_panel_rvq_launch(const void* A, const void* B, const void* M, const void* P, int64_t m, int c,
                          const void* grid_packed_abs, const void* resid_grid, float resid_scale, void* hat, void* idx,
                          hipStream_t stream) {
  if (m <= 0) return QUIP_OK;
  if (c < 8 || c % 8 != 0 || c > kPanelMaxCols) return QUIP_ERR_BAD_SHAPE;
  const int64_t blocks = (m + kPanelRows - 1) / kPanelRows;
  if (blocks > 0x7fffffff) return QUIP_ERR_BAD_SHAPE;
  auto go = [&](auto k, int step) {
    return launch<decltype(k)::value>(dim3((unsigned)blocks), dim3(256), ldlq_panel_lds_bytes(c, step), stream,
                                      reinterpret_cast<const float*>(A), reinterpret_cast<const float*>(B),
                                      reinterpret_cast<const float*>(M), reinterpret_cast<const float*>(P), m, c,
                                      reinterpret_cast<const uint64_t*>(grid_packed_abs),
                                      reinterpret_cast<const float*>(resid_grid), resid_scale,
                                      reinterpret_cast<float*>(hat), reinterpret_cast<int64_t*>(idx));
  };
  return resid_grid == nullptr ? go(kernel_c<ldlq_panel_kernel<kStepRVQ4>>, kStepRVQ4)
                               : go(kernel_c<ldlq_panel_kernel<kStepRVQ3>>, kStepRVQ3);
}

}  // namespace quip
