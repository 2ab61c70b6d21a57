// The tile body of the skinny products: one column tile (CB column blocks of 32) of one matrix, as the header of
// e8p_skinny_gemm.hip describes it.  Three kernels are made of it: e8p_skinny_gemm_kernel (e8p_skinny_gemm.hip: one tile
// per workgroup, WALK = 0), e8p_skinny_group_kernel (e8p_skinny_group.hip: a workgroup walks tiles of 1..3 matrices whose
// operands the host names, WALK = 1) and e8p_skinny_moe_kernel (e8p_skinny_moe.hip: a workgroup walks tiles of the experts
// that own rows, and reads a tile's rows, codes and row count on the device, WALK = 2).  Per tile all issue the same
// requests in the same order and add the K slices in the same order, so a column's fp32 sum does not depend on which of
// them computed it.  (The walk of e8p_skinny_moe_kernel was added to this template -- its preamble, its per-tile operands, its
// epilogue branch and the loop's condition sit behind `if constexpr (WALK == 2)` -- so the two older kernels are compiled
// from a changed template; their WALK 0 / 1 paths read as before.)
#pragma once
#include "quip_device.hip.h"
#include "launch.hip.h"
#include <type_traits>

namespace quip {

namespace {

typedef _Float16 sf16x8 __attribute__((ext_vector_type(8)));
typedef float sf32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t su32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t su32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t su32x3 __attribute__((ext_vector_type(3)));

constexpr int kSRep = 16;
constexpr int kST1 = 0;
constexpr int kST2 = 256 * kSRep * 8;        // 32 KiB
constexpr int kSRed = 2 * kST2;              // 64 KiB; behind the tables: the granule rings (16 waves x 3 x 2 KiB), later
                                             // the reduction (16 waves x 16 registers x 64 lanes fp32 = 64 KiB)
constexpr int kSLds = kSRed + 16 * 3 * 2048;      // 160 KiB

struct ST2Image {
  uint2 v[256];
  constexpr ST2Image() : v{} {
    for (int s = 0; s < 256; ++s) {
      int par = 0;
      for (int b = 0; b < 8; ++b) par ^= (s >> b) & 1;
      const int sv = s ^ par;
      uint32_t lo = 0, hi = 0;
      for (int p = 0; p < 4; ++p) {
        lo |= (((sv >> (7 - e8p_byte_of_pos(p))) & 1) ? 0xfcu : 0u) << (8 * p);
        hi |= (((sv >> (7 - e8p_byte_of_pos(p + 4))) & 1) ? 0xfcu : 0u) << (8 * p);
      }
      const uint32_t sh = par ? 0x02020202u : 0u;
      v[s].x = lo ^ sh;
      v[s].y = hi ^ sh;
    }
  }
};
__device__ const ST2Image kST2Img{};

__device__ __forceinline__ uint2 s_lds_read8(uint32_t addr) {
  const su32x2 v = *reinterpret_cast<const __attribute__((address_space(3))) su32x2*>((uintptr_t)addr);
  return make_uint2(v.x, v.y);
}

__device__ __forceinline__ void s_bytes_to_f16x4(uint32_t u4, uint32_t& lo, uint32_t& hi) {
  const uint32_t k5c = 0x5c5c5c5cu;
  const uint32_t a = __builtin_amdgcn_perm(u4, k5c, 0x00050004u);   // [u0, 5c, u1, 5c]
  const uint32_t b = __builtin_amdgcn_perm(u4, k5c, 0x00070006u);   // [u2, 5c, u3, 5c]
  const f16x2 m288 = {(f16)-288.f, (f16)-288.f};
  lo = as_u32(as_f16x2(a) + m288);
  hi = as_u32(as_f16x2(b) + m288);
}

constexpr int kSDepth = 3;   // granules in flight per wave

// 1..3 products of one codebook, M and K for e8p_skinny_group_kernel, by value in the kernel arguments.  A tile is
// 32 CB columns of one problem; problem g owns tiles [tile0[g], tile0[g + 1]), tile0[3] = all of them (a problem that
// is not there has no tiles and repeats the pointers of problem 0)
struct SkinnyGroupArgs {
  const f16* x[3];
  const uint16_t* q[3];
  f16* y[3];
  int n[3];
  int tile0[4];
  int M, K;
  const uint64_t* grid;
  const uint32_t* grid2;
  float resid_scale;
};

// The routed products of e8p_skinny_moe_kernel: 1..2 stacks of E code matrices (N, K), the rows of X[g] sorted by expert.
// Expert e owns rows [start[e], start[e + 1]) of every X[g] / Y[g]; start lives on the device, so the launch is the same
// whichever experts the rows chose.  Y[g][s] = fp16(scale[g, e] * fp16(X[g][s] . decode(q[g][e])))
struct SkinnyMoeArgs {
  const f16* x;              // (G, P, K)
  const uint16_t* q[2];      // (E, N, K / 8) each
  f16* y;                    // (G, P, N)
  const int* start;          // (E + 1)
  const float* scale;        // (G, E)
  int G, E, P, N;
  int M;                     // no expert owns more rows than this (MP was chosen for it)
};

// CB column blocks of 32 per workgroup, 16 / CB slices of K (16 waves); MP = activation rows staged (16 or 32).
// WALK = 0 (false): the tile (X, Wc, Y, N, first column col0), M <= 32 rows.  WALK = 1 (true): the tiles blockIdx.x,
// blockIdx.x + gridDim.x, ... of *ga; the tables are built for the first of them and stay.  WALK = 2: the same walk over
// the tiles of *ma, numbered (g, j-th expert that owns rows, column tile) with the column tile fastest
template <int CB, int MP, int MODE, int WALK>
__device__ __forceinline__ void skinny_tiles(const f16* __restrict__ X, const uint16_t* __restrict__ Wc,
                                             const uint64_t* __restrict__ grid, f16* __restrict__ Y, int M, int N, int K,
                                             float resid_scale, const uint32_t* __restrict__ grid2, int col0,
                                             const SkinnyGroupArgs* ga, const SkinnyMoeArgs* ma = nullptr) {
  constexpr bool GROUP = WALK != 0;
  static_assert(WALK != 2 || MODE == 0, "the routed walk addresses E8P12 code rows (K / 8 x 2 bytes)");
  constexpr int NCL = (MODE == 1 || MODE == 3 || MODE == 4) ? 2 : 1;     // code loads per lane and unit (16 bytes; MODE 4: 12)
  constexpr int kRep2 = MODE == 4 ? 8 : kSRep;                           // copies of the sign table
  constexpr int kST3 = kST2 + 256 * 8 * 8;                               // MODE 4: the residual table (256 x 4 bytes x 16 copies)
  using CodeT = std::conditional_t<MODE == 4, su32x3, su32x4>;           // what one code load writes
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NKS = 16 / CB;
  constexpr int L = MP / 16;                 // load instructions per granule
  constexpr int kGran = MP * 64;             // bytes of a granule: MP rows x 32 k
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = wave % CB, ks = wave / CB;
  const int n = lane & 31, kb = lane >> 5;
  int tile = (int)blockIdx.x;
  // WALK 2: which experts own rows (lane e looks at expert e, E <= 64), the tiles there are, the epilogue's scale
  uint64_t moe_mask = 0;
  int moe_ne = 0, moe_ctiles = 1, moe_tiles = 0;
  float moe_scale = 1.f;
  if constexpr (WALK == 2) {
    const int rows_e = lane < ma->E ? ma->start[lane + 1] - ma->start[lane] : 0;
    moe_mask = __ballot(rows_e > 0);
    moe_ne = __popcll(moe_mask);
    moe_ctiles = (ma->N + 32 * CB - 1) / (32 * CB);
    moe_tiles = ma->G * moe_ne * moe_ctiles;
    if (tile >= moe_tiles) return;     // (the grid is sized for every expert: the workgroups beyond have no tile)
  }
  bool more = false;
  do {     // GROUP: the tiles of this workgroup; else left after the one tile
  if constexpr (WALK == 2) {
    // an empty expert has no tile: nothing of it is requested.  All of this is uniform (scalar loads and selects)
    const int ge = tile / moe_ctiles;
    const int g = ge >= moe_ne ? 1 : 0;
    uint64_t mk = moe_mask;
    for (int i = ge - g * moe_ne; i > 0; --i) mk &= mk - 1;
    const int e = __builtin_ctzll(mk);
    // clamped so that whatever `start` holds, rows [s0, s0 + M) lie inside the P rows of X[g] and Y[g]
    const int s0 = min(max(ma->start[e], 0), ma->P - 1);
    M = min(max(ma->start[e + 1] - s0, 1), min(ma->M, ma->P - s0));
    N = ma->N;
    X = ma->x + ((size_t)g * ma->P + s0) * K;
    Y = ma->y + ((size_t)g * ma->P + s0) * N;
    Wc = (g == 0 ? ma->q[0] : ma->q[1]) + (size_t)e * N * (K >> 3);
    col0 = (tile - ge * moe_ctiles) * (32 * CB);
    moe_scale = ma->scale[g * ma->E + e];
  }
  if constexpr (WALK == 1) {
    // (scalar selects, not indexed: the group stays in the kernel arguments)
    const int g = (tile >= ga->tile0[1] ? 1 : 0) + (tile >= ga->tile0[2] ? 1 : 0);
    X = g == 0 ? ga->x[0] : g == 1 ? ga->x[1] : ga->x[2];
    Wc = g == 0 ? ga->q[0] : g == 1 ? ga->q[1] : ga->q[2];
    Y = g == 0 ? ga->y[0] : g == 1 ? ga->y[1] : ga->y[2];
    N = g == 0 ? ga->n[0] : g == 1 ? ga->n[1] : ga->n[2];
    col0 = (tile - (g == 0 ? ga->tile0[0] : g == 1 ? ga->tile0[1] : ga->tile0[2])) * (32 * CB);
  }
  // the tables are built beside the first tile's requests
  const bool build = !GROUP || tile == (int)blockIdx.x;
  // the lane number as the prologue reads it.  GROUP: opaque per tile, so that what the prologue derives from it (the
  // table build's sixteen addresses, the row offsets) is worked out again for every tile instead of being kept in
  // registers across the K loop -- the kernel has 128 of them
  int lane_p = lane;
  if constexpr (GROUP) asm volatile("" : "+v"(lane_p));
  const int ncol = col0 + cb * 32 + (lane_p & 31);
  // K slice of this wave in units of 128 k: the first (units % NKS) slices get one unit more
  const int units = K >> 7;
  const int ubase = units / NKS, uextra = units - ubase * NKS;
  const int u0 = ks * ubase + min(ks, uextra), un = ubase + (ks < uextra ? 1 : 0);
  const int ulast = max(un - 1, 0), qlast = max(4 * un - 1, 0);

  // (a wave without units -- K < 2048 -- still issues the loads of the prologue: inside its row)
  // a unit's 16 codes of a column: 32 bytes (MODE 0), 64 bytes (MODE 1); lane kb takes the half with blocks 8 kb .. 8 kb + 7
  // (MODE 4: a unit's 16 codes are 48 bytes; lane kb takes bytes [24 kb, 24 kb + 24) as two 12-byte loads)
  const char* wsrc_b = reinterpret_cast<const char*>(Wc) +
                       (MODE == 4 ? (size_t)min(ncol, N - 1) * (size_t)(K >> 3) * 3 + (size_t)48 * min(u0, units - 1) + 24 * (lane_p >> 5)
                                  : ((size_t)min(ncol, N - 1) * (K >> 3) * 2 * NCL + (size_t)32 * NCL * min(u0, units - 1) + 16 * NCL * (lane_p >> 5)));
  auto load_codes = [&](CodeT (&dst)[NCL], int u) {
#pragma unroll
    for (int c = 0; c < NCL; ++c) {
      if constexpr (MODE == 4)
        asm volatile("global_load_dwordx3 %0, %1, off" : "=v"(dst[c]) : "v"(wsrc_b + 48 * u + 12 * c) : "memory");
      else
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst[c]) : "v"(wsrc_b + 32 * NCL * u + 16 * c) : "memory");
    }
  };
  // granule loader: instruction h fills LDS slots [64 h, 64 h + 64) of the granule; slot s = (row s >> 2, stored
  // piece s & 3) holds source piece (s & 3) ^ ((row >> 1) & 3) of that row's 64 bytes
  const f16* xsrc[L];
#pragma unroll
  for (int h = 0; h < L; ++h) {
    const int row = 16 * h + (lane_p >> 2);
    const int p = (lane_p & 3) ^ ((row >> 1) & 3);
    xsrc[h] = X + (size_t)min(row, M - 1) * K + (size_t)min(u0, units - 1) * 128 + p * 8;
  }
  const uint32_t ring = (uint32_t)kSRed + (uint32_t)wave * (kSDepth * kGran);
  auto issue_x = [&](int q, int buf) {
#pragma unroll
    for (int h = 0; h < L; ++h)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(xsrc[h] + (size_t)q * 32),
          (__attribute__((address_space(3))) void*)(smem + ring + buf * kGran + h * 1024), 16, 0, 0);
  };

  // request order: the table source first (every wave asks, waves 0..7 use it: a load and its wait on the same
  // unconditional path keep the counting simple), then the codes of the first two units -- the table build below
  // waits for its source only, the codes stay in flight across it
  const bool second = (lane_p & 32) != 0;
  const int e = (wave & 7) * 32 + (lane_p & 31);
  su32x2 rawv;
  if (build) {
    const uint2* tsrc = (second || MODE == 3) ? &kST2Img.v[e] : reinterpret_cast<const uint2*>(grid) + e;   // (HI: no table, `grid` is not read)
    if (MODE == 4 && wave >= 8) tsrc = reinterpret_cast<const uint2*>(grid2 + (e & ~1));            // residual table: entries e & ~1, e | 1
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(rawv) : "v"(tsrc) : "memory");
  }
  // A register that a load is still going to write must never be a TIED asm operand ("+v") or cross a loop edge:
  // for either the compiler may emit a copy of it -- before the wait.  Loaded values are taken over by an asm that
  // waits and then moves them into fresh registers; only those are used afterwards.  (tools/check_inflight.py walks
  // the ISA for exactly this; tests/test_build_invariants.py runs it.)
  CodeT f0[NCL], f1[NCL], c2[NCL];
  load_codes(f0, 0);
  load_codes(f1, min(1, ulast));
  auto take = [](CodeT (&dst)[NCL], const CodeT (&src)[NCL], auto nw) {
#pragma unroll
    for (int c = 0; c < NCL; ++c) {
      if constexpr (MODE == 4)
        asm volatile("s_waitcnt vmcnt(%6)\n\tv_mov_b32 %0, %3\n\tv_mov_b32 %1, %4\n\tv_mov_b32 %2, %5"
                     : "=&v"(dst[c].x), "=&v"(dst[c].y), "=&v"(dst[c].z)
                     : "v"(src[c].x), "v"(src[c].y), "v"(src[c].z), "n"(decltype(nw)::value)
                     : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%8)\n\tv_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"
                     : "=&v"(dst[c].x), "=&v"(dst[c].y), "=&v"(dst[c].z), "=&v"(dst[c].w)
                     : "v"(src[c].x), "v"(src[c].y), "v"(src[c].z), "v"(src[c].w), "n"(decltype(nw)::value)
                     : "memory");
    }
  };
  // tables: T1' = (4a | 1) ^ 0x80.., T2 = sign masks; 16 copies each (waves 0..7)
  uint2 raw;
  if (build)
    asm volatile("s_waitcnt vmcnt(%4)\n\tv_mov_b32 %0, %2\n\tv_mov_b32 %1, %3"
                 : "=&v"(raw.x), "=&v"(raw.y)
                 : "v"(rawv.x), "v"(rawv.y), "n"(2 * NCL)
                 : "memory");
  if (!build) {
    // (a later tile of the group: the tables stand)
  } else if (wave < 8) {
    const uint32_t t1x = (__builtin_amdgcn_perm(0u, raw.x, 0x03010200u) | 0x01010101u) ^ 0x80808080u;
    const uint32_t t1y = (__builtin_amdgcn_perm(0u, raw.y, 0x03010200u) | 0x01010101u) ^ 0x80808080u;
    const su32x2 val = {(second || MODE == 2) ? raw.x : t1x, (second || MODE == 2) ? raw.y : t1y};   // (D4: the fp16 entries as they are)
    const uint32_t rowbase = (second ? (uint32_t)kST2 + (uint32_t)e * (kRep2 * 8) : (uint32_t)kST1 + (uint32_t)e * (kSRep * 8));
#pragma unroll
    for (int c = 0; c < kSRep; ++c) {
      const uint32_t copy = (uint32_t)(lane_p + c) & (uint32_t)((second ? kRep2 : kSRep) - 1);
      if (!second || c < kRep2)
        *reinterpret_cast<__attribute__((address_space(3))) su32x2*>((uintptr_t)(rowbase + copy * 8)) = val;
    }
  } else if (MODE == 4 && !second) {
    // waves 8..15, lanes 0..31: residual entry e = 32 (wave & 7) + lane, 16 copies of 4 bytes
    const uint32_t val = (e & 1) ? raw.y : raw.x;
    const uint32_t rowbase = (uint32_t)kST3 + (uint32_t)e * (kSRep * 4);
#pragma unroll
    for (int c = 0; c < kSRep; ++c)
      *reinterpret_cast<__attribute__((address_space(3))) uint32_t*>((uintptr_t)(rowbase + (((uint32_t)(lane_p + c) & (kSRep - 1)) << 2))) = val;
  }
  __builtin_amdgcn_sched_barrier(0);
  // (a wave without units requests its three granules like the others: clamped addresses, never read)
#pragma unroll
  for (int q = 0; q < kSDepth; ++q) issue_x(min(q, qlast), q);
  __builtin_amdgcn_sched_barrier(0);
  using std::integral_constant;
  // the codes of units 0 and 1 have arrived (the granules were requested after them); tables written
  CodeT c0[NCL], c1[NCL];
  take(c0, f0, integral_constant<int, kSDepth * L>{});
  take(c1, f1, integral_constant<int, kSDepth * L>{});
  if (build) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  const uint32_t lane_c1 = (uint32_t)(lane & 15) << 3;
  const uint32_t lane_c2 = (MODE == 4 ? (uint32_t)(lane & 7) << 3 : lane_c1) | (uint32_t)kST2;
  const uint32_t lane_c3 = ((uint32_t)(lane & 15) << 2) | (uint32_t)kST3;
  // A fragment of MFMA t of a granule: row lane & 31, piece 2 kb + t
  const int arow = n & (MP - 1);
  const uint32_t rd0 = ring + (uint32_t)(arow * 64 + (((2 * kb + 0) ^ ((arow >> 1) & 3)) << 4));
  const uint32_t rd1 = ring + (uint32_t)(arow * 64 + (((2 * kb + 1) ^ ((arow >> 1) & 3)) << 4));

  sf32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // one granule: wait for it (NW = vector-memory operations issued after it), two MFMAs from code pair d
  auto granule = [&](uint32_t d, uint32_t boff, auto nw) {
    constexpr int NW = decltype(nw)::value;
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW) : "memory");
    su32x4 A0, A1;
    su32x2 t1a, t2a, t1b, t2b;
    const uint32_t a1 = ((d >> 1) & 0x7f80u) | lane_c1, a2 = ((d << 7) & 0x7f80u) | lane_c2;
    const uint32_t b1 = ((d >> 17) & 0x7f80u) | lane_c1, b2 = ((d >> 9) & 0x7f80u) | lane_c2;
    asm volatile("ds_read_b64 %0, %1" : "=v"(t1a) : "v"(a1));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t2a) : "v"(a2));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A0) : "v"(rd0 + boff));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t1b) : "v"(b1));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t2b) : "v"(b2));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A1) : "v"(rd1 + boff));
    asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(t1a), "+v"(t2a), "+v"(A0));
    uint32_t w0, w1, w2, w3;
    s_bytes_to_f16x4(t1a.x ^ t2a.x, w0, w1);
    s_bytes_to_f16x4(t1a.y ^ t2a.y, w2, w3);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A0),
                                                 __builtin_bit_cast(sf16x8, su32x4{w0, w1, w2, w3}), acc, 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t1b), "+v"(t2b), "+v"(A1));
    s_bytes_to_f16x4(t1b.x ^ t2b.x, w0, w1);
    s_bytes_to_f16x4(t1b.y ^ t2b.y, w2, w3);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A1),
                                                 __builtin_bit_cast(sf16x8, su32x4{w0, w1, w2, w3}), acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  // MODE 1: two 32-bit codes (main << 16 | residual) of this lane's two MFMAs
  const f16 rs16 = (f16)resid_scale;
  const f16x2 rs2 = {rs16, rs16};
  auto granule_rvq = [&](uint32_t dA, uint32_t dB, uint32_t boff, auto nw) {
    constexpr int NW = decltype(nw)::value;
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW) : "memory");
    su32x4 A0, A1;
    su32x2 t[8];
    auto addr = [&](uint32_t d, uint32_t (&a)[4]) {
      a[0] = ((d >> 17) & 0x7f80u) | lane_c1;     // main (high half): abs index, sign byte
      a[1] = ((d >> 9) & 0x7f80u) | lane_c2;
      a[2] = ((d >> 1) & 0x7f80u) | lane_c1;      // residual (low half)
      a[3] = ((d << 7) & 0x7f80u) | lane_c2;
    };
    uint32_t aa[4], ab[4];
    addr(dA, aa);
    addr(dB, ab);
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("ds_read_b64 %0, %1" : "=v"(t[i]) : "v"(aa[i]));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A0) : "v"(rd0 + boff));
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("ds_read_b64 %0, %1" : "=v"(t[4 + i]) : "v"(ab[i]));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A1) : "v"(rd1 + boff));
    auto weights = [&](const su32x2& m1, const su32x2& m2, const su32x2& r1, const su32x2& r2) -> su32x4 {
      uint32_t m[4], r[4], w[4];
      s_bytes_to_f16x4(m1.x ^ m2.x, m[0], m[1]);
      s_bytes_to_f16x4(m1.y ^ m2.y, m[2], m[3]);
      s_bytes_to_f16x4(r1.x ^ r2.x, r[0], r[1]);
      s_bytes_to_f16x4(r1.y ^ r2.y, r[2], r[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = as_u32(__builtin_elementwise_fma(rs2, as_f16x2(r[i]), as_f16x2(m[i])));
      return su32x4{w[0], w[1], w[2], w[3]};
    };
    asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(A0));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A0),
                                                 __builtin_bit_cast(sf16x8, weights(t[0], t[1], t[2], t[3])), acc, 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]), "+v"(A1));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A1),
                                                 __builtin_bit_cast(sf16x8, weights(t[4], t[5], t[6], t[7])), acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  // MODE 4: dwords (main << 16 | residual index << 8) of this lane's two MFMAs
  auto granule_rvq3 = [&](uint32_t dA, uint32_t dB, uint32_t boff, auto nw) {
    constexpr int NW = decltype(nw)::value;
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW) : "memory");
    su32x4 A0, A1;
    su32x2 t[4];
    uint32_t r[2];
    auto addr = [&](uint32_t d, uint32_t (&a)[3]) {
      a[0] = ((d >> 17) & 0x7f80u) | lane_c1;     // main: abs index (16 copies x 8 bytes), sign byte (8 copies)
      a[1] = ((d >> 10) & 0x3fc0u) | lane_c2;
      a[2] = ((d >> 2) & 0x3fc0u) | lane_c3;      // residual index (16 copies x 4 bytes)
    };
    uint32_t aa[3], ab[3];
    addr(dA, aa);
    addr(dB, ab);
    asm volatile("ds_read_b64 %0, %1" : "=v"(t[0]) : "v"(aa[0]));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t[1]) : "v"(aa[1]));
    asm volatile("ds_read_b32 %0, %1" : "=v"(r[0]) : "v"(aa[2]));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A0) : "v"(rd0 + boff));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t[2]) : "v"(ab[0]));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t[3]) : "v"(ab[1]));
    asm volatile("ds_read_b32 %0, %1" : "=v"(r[1]) : "v"(ab[2]));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A1) : "v"(rd1 + boff));
    auto weights = [&](const su32x2& m1, const su32x2& m2, uint32_t c) -> su32x4 {
      uint32_t m[4], w[4];
      s_bytes_to_f16x4(m1.x ^ m2.x, m[0], m[1]);
      s_bytes_to_f16x4(m1.y ^ m2.y, m[2], m[3]);
      const f16x2 half2 = {(f16)0.5f, (f16)0.5f}, m12 = {(f16)-12.f, (f16)-12.f};
      const uint32_t sh[4] = {c << 6, c << 2, c >> 2, c >> 6};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // nibble n = int4 of 2 x value: 0x4c00 | (n ^ 8) << 6 is 16 + (n ^ 8); x 0.5 - 12 = 0.5 ((n ^ 8) - 8), exact
        const f16x2 res = __builtin_elementwise_fma(as_f16x2((sh[i] & 0x03c003c0u) ^ 0x4e004e00u), half2, m12);
        w[i] = as_u32(__builtin_elementwise_fma(rs2, res, as_f16x2(m[i])));
      }
      return su32x4{w[0], w[1], w[2], w[3]};
    };
    asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(t[0]), "+v"(t[1]), "+v"(r[0]), "+v"(A0));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A0),
                                                 __builtin_bit_cast(sf16x8, weights(t[0], t[1], r[0])), acc, 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[2]), "+v"(t[3]), "+v"(r[1]), "+v"(A1));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A1),
                                                 __builtin_bit_cast(sf16x8, weights(t[2], t[3], r[1])), acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  // MODE 2: dword d = the four D4 code bytes of this lane's two MFMAs (two per MFMA: weights 0..3, 4..7 of the block)
  auto granule_d4 = [&](uint32_t d, uint32_t boff, auto nw) {
    constexpr int NW = decltype(nw)::value;
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW) : "memory");
    su32x4 A0, A1;
    su32x2 t[4];
    const uint32_t a0 = ((d << 7) & 0x7f80u) | lane_c1, a1 = ((d >> 1) & 0x7f80u) | lane_c1;
    const uint32_t a2 = ((d >> 9) & 0x7f80u) | lane_c1, a3 = ((d >> 17) & 0x7f80u) | lane_c1;
    asm volatile("ds_read_b64 %0, %1" : "=v"(t[0]) : "v"(a0));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t[1]) : "v"(a1));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A0) : "v"(rd0 + boff));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t[2]) : "v"(a2));
    asm volatile("ds_read_b64 %0, %1" : "=v"(t[3]) : "v"(a3));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A1) : "v"(rd1 + boff));
    asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(t[0]), "+v"(t[1]), "+v"(A0));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A0),
                                                 __builtin_bit_cast(sf16x8, su32x4{t[0].x, t[0].y, t[1].x, t[1].y}), acc, 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[2]), "+v"(t[3]), "+v"(A1));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A1),
                                                 __builtin_bit_cast(sf16x8, su32x4{t[2].x, t[2].y, t[3].x, t[3].y}), acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  // MODE 3: two 32-bit HI codes; nibble i of a code is column [0,2,4,6,1,3,5,7][i] of its 8-group, i.e. the fp16 pair d of
  // the fragment is (nibble d, nibble d + 4) (quip_device.hip.h: hi_decode_f16)
  auto granule_hi = [&](uint32_t dA, uint32_t dB, uint32_t boff, auto nw) {
    constexpr int NW = decltype(nw)::value;
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NW) : "memory");
    su32x4 A0, A1;
    asm volatile("ds_read_b128 %0, %1" : "=v"(A0) : "v"(rd0 + boff));
    asm volatile("ds_read_b128 %0, %1" : "=v"(A1) : "v"(rd1 + boff));
    auto weights = [&](uint32_t c) -> su32x4 {
      // 0x4c00 | n << 6 is the fp16 number 16 + n (the mantissa bit of weight 1.0 at exponent 4); 23.5 is a fp16 number too,
      // so the subtraction is exact (1024 + n would not do: 1031.5 is not representable)
      const f16x2 off = {(f16)-23.5f, (f16)-23.5f};
      const uint32_t sh[4] = {c << 6, c << 2, c >> 2, c >> 6};
      uint32_t w[4];
#pragma unroll
      for (int dd = 0; dd < 4; ++dd) w[dd] = as_u32(as_f16x2((sh[dd] & 0x03c003c0u) | 0x4c004c00u) + off);
      return su32x4{w[0], w[1], w[2], w[3]};
    };
    const su32x4 B0 = weights(dA), B1 = weights(dB);
    asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(A0));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A0), __builtin_bit_cast(sf16x8, B0), acc, 0, 0, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(A1));
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sf16x8, A1), __builtin_bit_cast(sf16x8, B1), acc, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  int rb = 0;                                   // ring buffer of the current granule
  auto next_rb = [&]() { rb = rb == kSDepth - 1 ? 0 : rb + 1; };
  for (int u = 0; u < un; ++u) {
    // the kb halves trade code pairs: afterwards c0.x / .z / .y / .w serve granules 0 / 1 / 2 / 3 (MODE 1: the dword
    // pairs (c0[0].x, .y) / (c0[1].x, .y) / (c0[0].z, .w) / (c0[1].z, .w))
    // (builtin, not asm: v_permlane32_swap has wait-state requirements against neighbouring VALU instructions that
    //  only the compiler's hazard recogniser keeps track of)
    uint32_t gA[4], gB[4];      // per granule: the code dword(s) of this lane
    if constexpr (MODE == 0 || MODE == 2) {
      const auto s01 = __builtin_amdgcn_permlane32_swap(c0[0].x, c0[0].y, false, false);
      const auto s23 = __builtin_amdgcn_permlane32_swap(c0[0].z, c0[0].w, false, false);
      gA[0] = s01[0]; gA[2] = s01[1]; gA[1] = s23[0]; gA[3] = s23[1];
      gB[0] = gB[1] = gB[2] = gB[3] = 0u;
    } else {
      su32x4 cd[2];
      if constexpr (MODE == 4) {
        // 12 landed bytes = four 3-byte codes [residual, e8p lo, e8p hi] -> dwords (main << 16 | residual << 8)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          cd[h] = su32x4{c0[h].x << 8, __builtin_amdgcn_perm(c0[h].y, c0[h].x, 0x0504030cu),
                         __builtin_amdgcn_perm(c0[h].z, c0[h].y, 0x0403020cu), c0[h].z & 0xffffff00u};
      } else {
        cd[0] = su32x4{c0[0].x, c0[0].y, c0[0].z, c0[0][3]};
        cd[1] = su32x4{c0[1].x, c0[1].y, c0[1].z, c0[1][3]};
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const auto sx = __builtin_amdgcn_permlane32_swap(cd[h].x, cd[h].z, false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(cd[h].y, cd[h].w, false, false);
        gA[h] = sx[0]; gB[h] = sy[0];           // granule h: blocks 4 h + 2 kb, + 1
        gA[2 + h] = sx[1]; gB[2 + h] = sy[1];   // granule 2 + h
      }
    }
    auto gran = [&](int i, auto nw) {
      if constexpr (MODE == 0) granule(gA[i], (uint32_t)(rb * kGran), nw);
      else if constexpr (MODE == 1) granule_rvq(gA[i], gB[i], (uint32_t)(rb * kGran), nw);
      else if constexpr (MODE == 2) granule_d4(gA[i], (uint32_t)(rb * kGran), nw);
      else if constexpr (MODE == 4) granule_rvq3(gA[i], gB[i], (uint32_t)(rb * kGran), nw);
      else granule_hi(gA[i], gB[i], (uint32_t)(rb * kGran), nw);
    };
    gran(0, integral_constant<int, 2 * L>{});
    load_codes(c2, min(u + 2, ulast));
    issue_x(min(4 * u + 3, qlast), rb);
    __builtin_amdgcn_sched_barrier(0);
    next_rb();
    gran(1, integral_constant<int, 2 * L + NCL>{});
    issue_x(min(4 * u + 4, qlast), rb);
    __builtin_amdgcn_sched_barrier(0);
    next_rb();
    gran(2, integral_constant<int, 2 * L + NCL>{});
    issue_x(min(4 * u + 5, qlast), rb);
    __builtin_amdgcn_sched_barrier(0);
    next_rb();
    gran(3, integral_constant<int, 2 * L>{});
    issue_x(min(4 * u + 6, qlast), rb);
    __builtin_amdgcn_sched_barrier(0);
    next_rb();
    // the codes of unit u + 2 were requested before granule 4u + 3, which has just been waited for
#pragma unroll
    for (int c = 0; c < NCL; ++c) c0[c] = c1[c];
    take(c1, c2, integral_constant<int, kSDepth * L>{});
  }
  // the trailing filler granules must have landed before the ring is reused for the reduction
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // the K slices of a column block, added in the order 0, 1, 2, ...: every wave reduces CB of the 16 accumulator
  // registers of one column block (deterministic, independent of scheduling)
  float* red = reinterpret_cast<float*>(smem + kSRed);
  int lane_r = lane;      // (GROUP: as lane_p, for the addresses of the exchange)
  if constexpr (GROUP) asm volatile("" : "+v"(lane_r));
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane_r] = acc[r];
  __syncthreads();
  {
    const int ocb = wave % CB, r0 = (wave / CB) * CB;      // output column block, first register of this wave
    const int ocol = col0 + ocb * 32 + (lane_r & 31);
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      const int r = r0 + i;
      float v = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < NKS; ++s2) v += red[((s2 * CB + ocb) * 16 + r) * 64 + lane_r];
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane_r >> 5);
      if constexpr (WALK == 2) {
        // the sum rounded as the single launch stores it, then the module's scale: an fp32 product, rounded to fp32, and
        // only then to fp16 (left to the compiler the two become one v_fma_mixlo_f16, which rounds once)
        float scaled = (float)(f16)v * moe_scale;
        asm volatile("" : "+v"(scaled));
        if (row < M && ocol < N) Y[(size_t)row * N + ocol] = (f16)scaled;
      } else {
        if (row < M && ocol < N) Y[(size_t)row * N + ocol] = (f16)v;
      }
    }
  }
  if constexpr (GROUP) {
    // the next tile's granules land where the sums were just read.  (This tile's stores stand at the head of the next
    // tile's queue: every count of the prologue leaves requests issued AFTER them in flight, so they only wait longer.)
    __syncthreads();
    tile += (int)gridDim.x;
  }
  if constexpr (WALK == 1) more = tile < ga->tile0[3];
  if constexpr (WALK == 2) more = tile < moe_tiles;
  } while (more);
}

}  // namespace

}  // namespace quip
