// The row-wise launches around the routed products of a sparse-MoE MLP (Mixtral) at 1 <= M <= 31 decode rows.  Part of
// e8p_skinny_moe.hip's translation unit.  Nothing here is read back by the host: which experts a row takes stays on the
// device, from the router to the residual add.
//
// moe_route_rows_kernel -- grid M, 1024 threads, workgroup b owns row b:
//   xn     = (h[r] * rms_scale(1, sum h[r]^2, hidden, eps)) * ln      fp32, the expressions of the norm fused into the
//            input transforms (had_device.hip.h)
//   logit  = fp16(sum_k xn[k] Wg[e, k])                               fp32 FMA per lane in increasing k, xor butterfly
//   w      = softmax over the E logits in fp32; the top_k largest LOGITS are taken (the fp16 values order exactly; two
//            distinct logits can round to one fp32 probability), the lower expert index on a tie; / their sum when renorm
//   sorted order "by expert, then by row": start[E + 1], pair_of[P], weight[P], P = M top_k (pair p = r top_k + slot)
//   xs[g, s, :] = fp16(xn[r] * SU_g[e, :]) at the sorted position s of each of the row's pairs, g < G <= 2 (no SU_g: ones)
//   The sorted position of a pair depends on every row's choice.  Instead of meeting the other workgroups at a grid-wide
//   barrier, EVERY workgroup routes all M rows itself: wave w takes rows w, w + 16, ... (M E dot products of `hidden`, h and
//   Wg from L2: 31 x 8 x 4096 for Mixtral), one thread per row does softmax and top-k out of LDS, one thread per expert
//   counts, one thread adds the prefix.  All workgroups run the same instructions on the same data, so they agree bit for
//   bit; no atomics, no counter to keep clean between the replays of a graph, no workgroup waits for another.  The order
//   is a pure function of the ids.  Workgroup b then writes only the entries of ITS pairs (and workgroup 0 `start`), so
//   every output element has one writer.  A row of NaN / inf gives NaN weights and NaN rows for its own pairs; its ids are
//   still top_k distinct experts (the lowest ones), so every index stays in range and no other row is touched.
//
// moe_combine_rows_kernel<MODE> -- grid (rows, column blocks of 256 x 8), 256 threads:
//   MODE 0, combine, one row r of M:  out[r] = fp16(residual[r] + sum_slots weight[s] * (SV[e(s)] (.) t[s])), fp32 FMA in
//     ascending slot order from 0; s = the position with pair_of[s] = r top_k + slot (the workgroup scans pair_of: P <= 248),
//     e(s) = the expert whose [start[e], start[e + 1]) holds s.  A row's bits depend on that row alone.
//   MODE 1, the middle of the MLP, one sorted position s of P:
//     out[s] = fp16((fp16(u[s] SVu[e]) * silu(fp16(g[s] SVg[e]))) * SUd[e]),   e = e(s)
//     -- what the experts' gate / up modules round their outputs to, the SiLU product of down_proj's fused input transform,
//     and down_proj's sign vector, in one pass.
#pragma once
#include "had_device.hip.h"
#include "launch.hip.h"
#include "quip_device.hip.h"

namespace quip {

constexpr int kMoeMaxExperts = 64, kMoeMaxRows = 31, kMoeMaxTopK = 8;

namespace {

constexpr int kMoeRouteWaves = 16;
constexpr int kMoeRowsThreads = 256;

struct MoeRouteArgs {
  const f16 *h, *ln, *wg, *su0, *su1;
  f16* xs;
  int *start, *pair_of;
  float* weight;
  int M, hidden, E, top_k, G, renorm;
  float eps;
};

__device__ __forceinline__ float moe_wave_sum(float s) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s = had::fadd(s, __shfl_xor(s, o, 64));
  return s;
}

__device__ __forceinline__ uint4 moe_pack8(const float v[8]) {
  const had::f32x2 o[4] = {{v[0], v[1]}, {v[2], v[3]}, {v[4], v[5]}, {v[6], v[7]}};
  return had::pack8p(o);
}

// fp16 rounding of a product, as a module's output transform stores it
__device__ __forceinline__ float moe_round_f16(float v) { return (float)(f16)v; }

__global__ __launch_bounds__(64 * kMoeRouteWaves) void moe_route_rows_kernel(const MoeRouteArgs a) {
  __shared__ float s_logit[kMoeMaxRows][kMoeMaxExperts];
  __shared__ float s_w[kMoeMaxRows][kMoeMaxTopK];
  __shared__ int s_id[kMoeMaxRows][kMoeMaxTopK];
  __shared__ float s_rs[kMoeMaxRows];
  __shared__ int s_start[kMoeMaxExperts + 1];
  __shared__ int s_pos[kMoeMaxTopK];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int pieces = a.hidden >> 3, E = a.E, M = a.M, top_k = a.top_k;
  const uint4* lnp = reinterpret_cast<const uint4*>(a.ln);
  const uint4* wgp = reinterpret_cast<const uint4*>(a.wg);

  // the router of every row: norm factor, E logits
  for (int r = wave; r < M; r += kMoeRouteWaves) {
    const uint4* xr = reinterpret_cast<const uint4*>(a.h + (size_t)r * a.hidden);
    float ss = 0.f;
    for (int p = lane; p < pieces; p += 64) {
      float v[8];
      had::unpack8(xr[p], v);
      had::sumsq8(v, ss);
    }
    const float rs = had::rms_scale(1.f, moe_wave_sum(ss), a.hidden, a.eps);
    if (lane == 0) s_rs[r] = rs;
    for (int e0 = 0; e0 < E; e0 += 4) {       // four experts per pass over the row
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int p = lane; p < pieces; p += 64) {
        float v[8], w[8];
        had::unpack8(xr[p], v);
        had::unpack8(lnp[p], w);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = had::fmul(had::fmul(v[i], rs), w[i]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float g[8];
          had::unpack8(wgp[(size_t)min(e0 + c, E - 1) * pieces + p], g);
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[c] = __builtin_fmaf(v[i], g[i], acc[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float l = moe_wave_sum(acc[c]);
        if (lane == 0 && e0 + c < E) s_logit[r][e0 + c] = moe_round_f16(l);
      }
    }
  }
  __syncthreads();

  // softmax and top-k: thread r takes row r
  if (tid < M) {
    const float* l = s_logit[tid];
    float mx = l[0];
    for (int e = 1; e < E; ++e) mx = fmaxf(mx, l[e]);
    float sum = 0.f;
    for (int e = 0; e < E; ++e) sum = had::fadd(sum, expf(had::fsub(l[e], mx)));
    uint64_t taken = 0;
    float wsum = 0.f;
    for (int j = 0; j < top_k; ++j) {
      int best = -1;
      float bl = 0.f;
      for (int e = 0; e < E; ++e)
        if (!((taken >> e) & 1) && (best < 0 || l[e] > bl)) {     // (strictly greater: the lower index keeps a tie)
          best = e;
          bl = l[e];
        }
      taken |= 1ull << best;
      const float w = expf(had::fsub(bl, mx)) / sum;
      s_id[tid][j] = best;
      s_w[tid][j] = w;
      wsum = had::fadd(wsum, w);
    }
    if (a.renorm)
      for (int j = 0; j < top_k; ++j) s_w[tid][j] = s_w[tid][j] / wsum;
  }
  __syncthreads();

  // rows per expert, then their prefix
  if (tid < E) {
    int c = 0;
    for (int r = 0; r < M; ++r)
      for (int j = 0; j < top_k; ++j) c += s_id[r][j] == tid ? 1 : 0;
    s_start[tid + 1] = c;
  }
  __syncthreads();
  if (tid == 0) {
    s_start[0] = 0;
    for (int e = 0; e < E; ++e) s_start[e + 1] += s_start[e];
  }
  __syncthreads();
  const int r0 = blockIdx.x;
  if (r0 == 0 && tid <= E) a.start[tid] = s_start[tid];
  if (tid < top_k) {
    // the pair's place: behind the earlier rows that chose the same expert (a row names an expert once)
    const int e = s_id[r0][tid];
    int s = s_start[e];
    for (int r = 0; r < r0; ++r)
      for (int j = 0; j < top_k; ++j) s += s_id[r][j] == e ? 1 : 0;
    a.pair_of[s] = r0 * top_k + tid;
    a.weight[s] = s_w[r0][tid];
    s_pos[tid] = s;
  }
  __syncthreads();

  // the signed rows of this row's pairs
  const uint4* xr = reinterpret_cast<const uint4*>(a.h + (size_t)r0 * a.hidden);
  const float rs = s_rs[r0];
  const int P = M * top_k;
  for (int idx = tid; idx < a.G * top_k * pieces; idx += 64 * kMoeRouteWaves) {
    const int p = idx % pieces, gj = idx / pieces, j = gj % top_k, g = gj / top_k;
    float v[8], w[8];
    had::unpack8(xr[p], v);
    had::unpack8(lnp[p], w);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = had::fmul(had::fmul(v[i], rs), w[i]);
    const f16* su = g == 0 ? a.su0 : a.su1;
    if (su) had::mul8(v, reinterpret_cast<const uint4*>(su)[(size_t)s_id[r0][j] * pieces + p]);
    reinterpret_cast<uint4*>(a.xs)[((size_t)g * P + s_pos[j]) * pieces + p] = moe_pack8(v);
  }
}

struct MoeRowsArgs {
  const f16 *t, *t2, *sv, *sv2, *su, *residual;
  f16* out;
  const int *start, *pair_of;
  const float* weight;
  int width, E, top_k, P;
};

// the expert that owns sorted position s (0 when `start` names none: every index stays in range)
__device__ __forceinline__ int moe_expert_of(const int* start, int E, int s) {
  int e = 0;
  for (int i = 0; i < E; ++i)
    if (start[i] <= s && s < start[i + 1]) e = i;
  return e;
}

template <int MODE>
__global__ __launch_bounds__(kMoeRowsThreads) void moe_combine_rows_kernel(const MoeRowsArgs a) {
  __shared__ int s_pos[kMoeMaxTopK], s_e[kMoeMaxTopK];
  __shared__ float s_w[kMoeMaxTopK];
  const int tid = threadIdx.x, row = blockIdx.x, pieces = a.width >> 3;
  const int p = blockIdx.y * kMoeRowsThreads + tid;
  if constexpr (MODE == 0) {
    if (tid < kMoeMaxTopK) s_pos[tid] = -1;
    __syncthreads();
    for (int s = tid; s < a.P; s += kMoeRowsThreads) {
      const int pr = a.pair_of[s];
      if (pr >= row * a.top_k && pr < (row + 1) * a.top_k) s_pos[pr - row * a.top_k] = s;
    }
    __syncthreads();
    if (tid < a.top_k && s_pos[tid] >= 0) {
      s_e[tid] = moe_expert_of(a.start, a.E, s_pos[tid]);
      s_w[tid] = a.weight[s_pos[tid]];
    }
    __syncthreads();
    if (p >= pieces) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.top_k; ++j) {
      const int s = s_pos[j];
      if (s < 0) continue;       // (a pair_of that is no permutation: the slot adds nothing)
      float v[8];
      had::unpack8(reinterpret_cast<const uint4*>(a.t)[(size_t)s * pieces + p], v);
      if (a.sv) had::mul8(v, reinterpret_cast<const uint4*>(a.sv)[(size_t)s_e[j] * pieces + p]);
      const float w = s_w[j];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(w, v[i], acc[i]);
    }
    if (a.residual) {
      float res[8];
      had::unpack8(reinterpret_cast<const uint4*>(a.residual)[(size_t)row * pieces + p], res);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = had::fadd(res[i], acc[i]);
    }
    reinterpret_cast<uint4*>(a.out)[(size_t)row * pieces + p] = moe_pack8(acc);
  } else {
    if (tid == 0) s_e[0] = moe_expert_of(a.start, a.E, row);
    __syncthreads();
    if (p >= pieces) return;
    const size_t at = (size_t)row * pieces + p, ate = (size_t)s_e[0] * pieces + p;
    float g[8], u[8];
    had::unpack8(reinterpret_cast<const uint4*>(a.t)[at], g);
    had::unpack8(reinterpret_cast<const uint4*>(a.t2)[at], u);
    if (a.sv) had::mul8(g, reinterpret_cast<const uint4*>(a.sv)[ate]);
    if (a.sv2) had::mul8(u, reinterpret_cast<const uint4*>(a.sv2)[ate]);
#pragma unroll
    for (int i = 0; i < 8; ++i) u[i] = had::fmul(moe_round_f16(u[i]), had::silu(moe_round_f16(g[i])));
    if (a.su) had::mul8(u, reinterpret_cast<const uint4*>(a.su)[ate]);
    reinterpret_cast<uint4*>(a.out)[at] = moe_pack8(u);
  }
}

}  // namespace

int moe_route_rows_launch(const void* h, const void* ln, const void* wg, const void* su0, const void* su1, void* xs,
                          int32_t* start, int32_t* pair_of, float* weight, int rows, int hidden, int experts, int top_k,
                          int stacks, int renorm, float eps, hipStream_t stream) {
  if (rows < 1 || hidden < 8 || hidden % 8 != 0 || experts < 1 || top_k < 1 || top_k > experts || stacks < 1 || stacks > 2)
    return QUIP_ERR_BAD_SHAPE;
  if (rows > kMoeMaxRows || experts > kMoeMaxExperts || top_k > kMoeMaxTopK) return QUIP_ERR_UNSUPPORTED;
  MoeRouteArgs a;
  a.h = reinterpret_cast<const f16*>(h);
  a.ln = reinterpret_cast<const f16*>(ln);
  a.wg = reinterpret_cast<const f16*>(wg);
  a.su0 = reinterpret_cast<const f16*>(su0);
  a.su1 = reinterpret_cast<const f16*>(su1);
  a.xs = reinterpret_cast<f16*>(xs);
  a.start = start; a.pair_of = pair_of; a.weight = weight;
  a.M = rows; a.hidden = hidden; a.E = experts; a.top_k = top_k; a.G = stacks; a.renorm = renorm; a.eps = eps;
  return launch<moe_route_rows_kernel>(dim3((unsigned)rows), dim3(64 * kMoeRouteWaves), 0, stream, a);
}

int moe_rows_launch(int mode, const void* t, const void* t2, const void* sv, const void* sv2, const void* su,
                    const void* residual, void* out, const int32_t* start, const int32_t* pair_of, const float* weight,
                    int rows, int width, int experts, int top_k, int pairs, hipStream_t stream) {
  if (rows < 1 || width < 8 || width % 8 != 0 || experts < 1 || top_k < 1 || top_k > experts || pairs < 1 ||
      rows != (mode == 0 ? pairs / top_k : pairs) || pairs % top_k != 0)
    return QUIP_ERR_BAD_SHAPE;
  if (pairs > kMoeMaxRows * top_k || experts > kMoeMaxExperts || top_k > kMoeMaxTopK) return QUIP_ERR_UNSUPPORTED;
  MoeRowsArgs a;
  a.t = reinterpret_cast<const f16*>(t);
  a.t2 = reinterpret_cast<const f16*>(t2);
  a.sv = reinterpret_cast<const f16*>(sv);
  a.sv2 = reinterpret_cast<const f16*>(sv2);
  a.su = reinterpret_cast<const f16*>(su);
  a.residual = reinterpret_cast<const f16*>(residual);
  a.out = reinterpret_cast<f16*>(out);
  a.start = start; a.pair_of = pair_of; a.weight = weight;
  a.width = width; a.E = experts; a.top_k = top_k; a.P = pairs;
  const int blocks = (width / 8 + kMoeRowsThreads - 1) / kMoeRowsThreads;
  const dim3 grid((unsigned)rows, (unsigned)blocks), block(kMoeRowsThreads);
  if (mode == 0) return launch<moe_combine_rows_kernel<0>>(grid, block, 0, stream, a);
  return launch<moe_combine_rows_kernel<1>>(grid, block, 0, stream, a);
}

}  // namespace quip
