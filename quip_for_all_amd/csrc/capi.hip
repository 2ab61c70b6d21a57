// extern "C" entry points of libquip_mi355.so (see include/quip_mi355.h).
// Argument validation lives here; the reference validated nothing
// (origin_order.cu:557-788 have no dtype / shape / contiguity checks).
#include <stdlib.h>

#include <initializer_list>

#include "launch.hip.h"

namespace quip {

int device_cu_count() {
  static int cached[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  if (cached[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    cached[dev] = v;
  }
  return cached[dev];
}

int device_cu_count_strict() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 0;
  return v;
}

bool persistent_grid_fits(ResidencyCache& cache, const void* kernel, int threads, int lds, int nwg) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const bool slot = dev >= 0 && dev < 16;
  if (slot && cache.ok[dev] != 0) return cache.ok[dev] > 0;
  bool fits = false;
  const int cus = device_cu_count_strict();
  int per_cu = 0;
  // (one workgroup per CU is the design -- the LDS footprint admits no second one --, so a device with fewer CUs than
  //  workgroups, e.g. a CPX partition or a CU-masked queue, cannot hold the grid whatever the occupancy query says)
  if (cus >= nwg && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, (size_t)lds) == hipSuccess)
    fits = (long long)per_cu * cus >= nwg;
  if (slot) cache.ok[dev] = fits ? 1 : -1;
  return fits;
}

int ensure_dyn_lds(DynLdsCache& cache, const void* kernel, int lds) {
  if (lds <= 48 * 1024) return QUIP_OK;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return QUIP_ERR_LAUNCH;
  const bool slot = dev >= 0 && dev < 16;
  if (slot && lds <= cache.bytes[dev]) return QUIP_OK;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return QUIP_ERR_LAUNCH;
  if (slot) cache.bytes[dev] = lds;
  return QUIP_OK;
}

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

static inline bool aligned64(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 63u) == 0; }

// pointer lists of an entry point's prologue
namespace {
using Ptrs = std::initializer_list<const void*>;
bool any_null(Ptrs ps) {
  for (const void* p : ps)
    if (!p) return true;
  return false;
}
bool any_off(Ptrs ps, uintptr_t mask) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & mask) return true;
  return false;
}

// ---- the products of the five codebooks ----------------------------------------------------------------------------------
// Four families serve the 20 per-codebook entries: original order (generic_mm_launch), skinny (skinny_gemm_launch), batched
// (prefill_gemm_launch) and decompress (decompress_launch).  An entry fills CodebookArgs and calls its family with its
// CodebookId; what a family asks of a codebook stands in this table, indexed by CodebookId.  What the families answer, and
// in which order, is pinned row by row in tests/golden/product_refusals.json.
struct ProductChecks {
  bool grid, grid2;             // the tables the codebook needs (NULL: QUIP_ERR_NULL_POINTER)
  int kdiv;                     // original order and decompress: k % kdiv (E8P12RVQ3B: rows of 3 k / 8 bytes, dword aligned)
  uintptr_t skinny_q_mask;      // skinny: alignment - 1 of the codes (the 3-byte codes: 4 bytes, else 16)
  // The packed E81B table is asked to be 8-byte aligned by the skinny family (as every table there) and 4-byte aligned by
  // the batched one (uint32 entries).  Both are ABI as recorded; DESIGN 9 item 12.
  uintptr_t skinny_grid2_mask, batched_grid2_mask;
  // quip_e8p_mm_batched accepts m == 0 before it looks at any alignment, as the skinny family does; the other four batched
  // entries look at the alignment first and accept m == 0 last.  ABI as recorded; DESIGN 9 item 12.
  bool batched_empty_first;
};
constexpr ProductChecks kProduct[5] = {
    /* kE8P     */ {true, false, 8, 15, 0, 0, true},
    /* kE8PRVQ3 */ {true, true, 32, 3, 7, 3, false},
    /* kE8PRVQ4 */ {true, false, 8, 15, 0, 0, false},
    /* kD4      */ {true, false, 8, 15, 0, 0, false},
    /* kHI      */ {false, false, 8, 15, 0, 0, false},
};
bool tables_null(const ProductChecks& c, const CodebookArgs& a) { return (c.grid && !a.grid) || (c.grid2 && !a.grid2); }

// original order: the tables, then x / qidxs / y, the shape, the empty product, x 16-byte aligned (nobody looks at the rest)
int mm_origorder(CodebookId cb, const void* x, const void* q, const CodebookArgs& a, void* y, int m, int n, int k,
                 quip_stream_t s) {
  const ProductChecks& c = kProduct[cb];
  if (tables_null(c, a) || any_null({x, q, y})) return QUIP_ERR_NULL_POINTER;
  if (m < 0 || n < 0 || k <= 0 || k % c.kdiv != 0 || k % 8 != 0) return QUIP_ERR_BAD_SHAPE;
  if (m == 0 || n == 0) return QUIP_OK;
  if (!aligned16(x)) return QUIP_ERR_MISALIGNED;
  return generic_mm_launch(cb, x, q, a, y, m, n, k, (hipStream_t)s);
}

int decompress_origorder(CodebookId cb, const void* q, const CodebookArgs& a, void* w, int64_t rows, int k, quip_stream_t s) {
  const ProductChecks& c = kProduct[cb];
  if (tables_null(c, a) || any_null({q, w})) return QUIP_ERR_NULL_POINTER;
  if (rows < 0 || k <= 0 || k % c.kdiv != 0 || k % 8 != 0) return QUIP_ERR_BAD_SHAPE;
  if (rows == 0) return QUIP_OK;
  if (!aligned16(w)) return QUIP_ERR_MISALIGNED;
  return decompress_launch(cb, q, a, w, rows, k, (hipStream_t)s);
}

// skinny (e8p_skinny_gemm.hip): x and the codes 16-byte aligned (the 3-byte codes: 4), y 4-byte, every table 8-byte; m == 0
// is accepted before the alignment is looked at (the caller returns, no launch)
int mm_skinny(CodebookId cb, const void* x, const void* q, const CodebookArgs& a, void* y, int m, int n, int k,
              quip_stream_t s) {
  const ProductChecks& c = kProduct[cb];
  if (any_null({x, q, y}) || tables_null(c, a)) return QUIP_ERR_NULL_POINTER;
  if (m < 0 || n < 1 || k < 8) return QUIP_ERR_BAD_SHAPE;
  if (m == 0) return QUIP_OK;
  if (any_off({x}, 15) || any_off({q}, c.skinny_q_mask) || any_off({y}, 3) || any_off({a.grid}, 7) ||
      any_off({a.grid2}, c.skinny_grid2_mask))
    return QUIP_ERR_MISALIGNED;
  return skinny_gemm_launch(cb, x, q, a, y, m, n, k, (hipStream_t)s);
}

// batched (e8p_prefill_gemm.hip): x, the codes and y 16-byte aligned, the E8P / D4 table 8-byte
int mm_batched(CodebookId cb, const void* x, const void* q, const CodebookArgs& a, void* y, int64_t m, int n, int k,
               quip_stream_t s) {
  const ProductChecks& c = kProduct[cb];
  if (tables_null(c, a) || any_null({x, q, y})) return QUIP_ERR_NULL_POINTER;
  if (m < 0 || n < 1 || k < 8) return QUIP_ERR_BAD_SHAPE;
  if (c.batched_empty_first && m == 0) return QUIP_OK;
  if (any_off({x, q, y}, 15) || any_off({a.grid}, 7) || any_off({a.grid2}, c.batched_grid2_mask)) return QUIP_ERR_MISALIGNED;
  if (m == 0) return QUIP_OK;
  return prefill_gemm_launch(cb, x, q, a, y, m, n, k, (hipStream_t)s);
}
}  // namespace

// ---- the stand-alone bs=1 GEMV -----------------------------------------------------------------------------------------
// Three kernels serve it: the first (e8p_gemv_mfma.hip: one-shot loads on 8 waves) and the K-splitting kernel
// (e8p_gemv_v2.hip: whole-line loads) with byte tables or in nibble mode (e8p_gemv_v2n.hip), each in one of three table
// modes (GemvTune::rep).  One argument check (gemv_launch) and one planner (gemv_plan) serve every entry point.
namespace {
struct GemvMode {
  int rep;              // 0 = E8P12, 64 = the D4 table (HI through its virtual layout), 40 = E8P12RVQ3B
  uintptr_t q_mask;     // Qidxs alignment - 1
  int k_multiple;
  uintptr_t grid_mask;  // grid alignment - 1 checked up front (0: left to the kernel that reads it)
  bool grid2;           // the E81B table (int8 (256, 8)), 8-byte aligned
  bool ws_required;     // a missing or short workspace: an error before the K-splitting kernel (else its own cue)
};
// E8P12RVQ3B: a 3-byte code behind a zero byte is (main16 << 16 | resid8 << 8), i.e. an RVQ4-style row of 2k virtual weights
// whose low 16-bit codes index the E81B table instead of the E8P tables; its rows are 3 k / 8 bytes, dword aligned
constexpr GemvMode kGemvE8P{0, 15, 8, 63, false, false};
constexpr GemvMode kGemvD4{64, 15, 8, 0, false, false};
constexpr GemvMode kGemvRVQ3{40, 3, 32, 0, true, true};

enum GemvKernel { kGemvFirst, kGemvV2Bytes, kGemvV2Nibble };
struct GemvPlan {
  GemvKernel kernel[3];
  int count = 0;
  void add(GemvKernel k) { kernel[count++] = k; }
};

// QUIP_GEMV_V2 = 0 / 1 forces the first / the K-splitting kernel for E8P12; QUIP_GEMV_NIB = 0 keeps the byte tables.
// Both are read once per process.
int gemv_v2_env() {
  static const int v = env_int("QUIP_GEMV_V2", -1);
  return v;
}
bool gemv_nibble_env() {
  static const bool v = env_int("QUIP_GEMV_NIB", 1) != 0;
  return v;
}

// nibble mode for rows whose digit image leaves the byte tables 16 copies only (k > 10240: two-way conflicts on every
// look-up; the nibble tables are 64 KB and conflict free whatever k is: 8192 x 28672 -5..9 % on two boxes, level on a third;
// at k = 8192 both are conflict free and the two kernels trade places from box to box: profiles/r06_gemv_v2_nibble.txt),
// and for grouped launches (q / k / v of 8192: 11.5-11.9 against 13.3 us and the first kernel's 12.4; gate / up 24.6
// against 27.5-28.2; at k = 4096 the byte tables win: 8.7 against 9.4 us for 2 x 11008)
bool gemv_prefers_nibble(int count, int k) { return gemv_nibble_env() && (k > 10240 || (count >= 2 && k >= 8192)); }

// the kernels a launch tries, in order (k: weights per row as the kernels see them).  E8P12 (measured on MI355X,
// tools/gemv_v2_bench.py): the K-splitting kernel wins from Llama-70B sizes on -- k >= 8192 with >= 16 MB of codes, or
// >= 20 MB of codes in the launch (7B gate / up group) -- and is the only one for rows longer than 28672 (E8P12RVQ4B's
// 2k-wide virtual rows at 70B); short launches stay on the first kernel.  The other table modes take the first kernel
// wherever it takes the shape (k <= 28672), else the K-splitting one (HI's / E8P12RVQ3B's virtual rows at the 70B
// down_proj width: 2 k = 57344; E8P12RVQ3B: one problem only)
GemvPlan gemv_plan(const GemvMode& mode, const int* ns, int count, int k) {
  GemvPlan p;
  if (mode.rep != 0) {
    p.add(kGemvFirst);
    if (mode.rep == 64 || count == 1) p.add(kGemvV2Bytes);
    return p;
  }
  size_t bytes = 0;
  for (int i = 0; i < count; ++i) bytes += (size_t)ns[i] * (size_t)k / 4;
  const bool first_ok = e8p_gemv_mfma_group_supported(ns, count, k);
  const int env = gemv_v2_env();
  if (env == 1 || !first_ok || (env != 0 && ((k >= 8192 && bytes >= ((size_t)16 << 20)) || bytes >= ((size_t)20 << 20)))) {
    if (gemv_prefers_nibble(count, k)) p.add(kGemvV2Nibble);
    p.add(kGemvV2Bytes);
  }
  if (first_ok) p.add(kGemvFirst);
  return p;
}

// the K-splitting kernel in the table mode of `t`; rep 0 takes nibble mode first where the planner would (unless the K
// split is forced), rep 4 nibble mode only
int gemv_v2_auto(const void* const* planes, const void* const* qidxs, const void* grid, void* const* ys, void* ws,
                 const int* ns, int count, int k, const GemvTune& t, hipStream_t stream) {
  if (t.rep == 0 && !t.waves_g && gemv_prefers_nibble(count, k)) {
    GemvTune tn = t;
    tn.rep = 4;
    const int rc = e8p_gemv_v2_group_launch(planes, qidxs, grid, ys, ws, ns, count, k, tn, stream);
    if (rc != QUIP_ERR_UNSUPPORTED && rc != QUIP_ERR_NULL_POINTER) return rc;
  }
  return e8p_gemv_v2_group_launch(planes, qidxs, grid, ys, ws, ns, count, k, t, stream);
}

int gemv_launch(const GemvMode& mode, const void* const* planes, const void* const* qidxs, const void* grid,
                const void* grid2, void* const* ys, const int32_t* ns, int32_t count, int32_t k, void* ws, size_t ws_bytes,
                quip_stream_t stream) {
  if (!planes || !qidxs || !grid || (mode.grid2 && !grid2) || !ys || !ns) return QUIP_ERR_NULL_POINTER;
  if (count < 1 || count > QUIP_MAX_GROUP) return QUIP_ERR_BAD_SHAPE;
  int n32[QUIP_MAX_GROUP];
  size_t need = 0;
  for (int i = 0; i < count; ++i) {
    if (!planes[i] || !qidxs[i] || !ys[i]) return QUIP_ERR_NULL_POINTER;
    if (!aligned16(planes[i]) || (reinterpret_cast<uintptr_t>(qidxs[i]) & mode.q_mask) != 0) return QUIP_ERR_MISALIGNED;
    if (ns[i] < 1) return QUIP_ERR_BAD_SHAPE;
    n32[i] = ns[i];
    need += e8p_gemv_v2_workspace_words(ns[i]) * 4;
  }
  if (k < 1 || k % mode.k_multiple != 0) return QUIP_ERR_BAD_SHAPE;
  if ((reinterpret_cast<uintptr_t>(grid) & mode.grid_mask) != 0 ||
      (mode.grid2 && (reinterpret_cast<uintptr_t>(grid2) & 7u) != 0) || (ws && !aligned16(ws)))
    return QUIP_ERR_MISALIGNED;
  if (ws_bytes < need) ws = nullptr;
  GemvTune t;
  t.rep = mode.rep;
  t.grid2 = mode.grid2 ? grid2 : nullptr;
  const int kv = mode.rep == 40 ? 2 * k : k;
  const GemvPlan plan = gemv_plan(mode, n32, count, kv);
  int rc = QUIP_ERR_UNSUPPORTED;
  // next kernel: after the first one on QUIP_ERR_UNSUPPORTED (it does not take the shape), after the K-splitting one also
  // on QUIP_ERR_NULL_POINTER (it needs a K split but has no workspace)
  for (int i = 0; i < plan.count; ++i) {
    if (plan.kernel[i] == kGemvFirst) {
      rc = e8p_gemv_mfma_group_launch(planes, qidxs, grid, ys, n32, count, kv, t, (hipStream_t)stream);
      if (rc != QUIP_ERR_UNSUPPORTED) return rc;
      continue;
    }
    if (mode.ws_required && !ws) return QUIP_ERR_NULL_POINTER;
    GemvTune tv = t;
    if (plan.kernel[i] == kGemvV2Nibble) tv.rep = 4;
    rc = e8p_gemv_v2_group_launch(planes, qidxs, grid, ys, ws, n32, count, kv, tv, (hipStream_t)stream);
    if (rc != QUIP_ERR_UNSUPPORTED && rc != QUIP_ERR_NULL_POINTER) return rc;
  }
  return rc;
}

// the tuning hooks' loose arguments (0: automatic) as the launchers' record
GemvTune tune_of(int rep, int rows, int blocks, int waves_g, int max_waves, int digits, void* dbg) {
  GemvTune t;
  t.rep = rep; t.rows = rows; t.blocks = blocks; t.waves_g = waves_g; t.max_waves = max_waves; t.digits = digits; t.dbg = dbg;
  return t;
}

// the public record of a fused GEMV's input side as the launcher's, the per-problem members for `count` problems
GemvFusedIn fused_in_of(const quip_gemv_fused_in* in, int count) {
  GemvFusedIn f;
  f.x = in->x; f.z = in->z; f.post = in->post_scale; f.residual = in->residual; f.h_out = in->h_out;
  f.rms_w = in->rms_weight; f.z_scale = in->z_scale; f.rms_eps = in->rms_eps;
  for (int i = 0; i < count && i < QUIP_MAX_GROUP; ++i) {
    f.pre[i] = in->pre_scale[i];
    f.scale[i] = in->scale[i];
  }
  return f;
}
}  // namespace

}  // namespace quip

using namespace quip;

extern "C" {

int quip_abi_version(void) { return QUIP_ABI_VERSION; }

const char* quip_strerror(int code) {
  switch (code) {
    case QUIP_OK: return "ok";
    case QUIP_ERR_NULL_POINTER: return "null pointer argument";
    case QUIP_ERR_BAD_SHAPE: return "shape not supported by the packed format";
    case QUIP_ERR_MISALIGNED: return "pointer not 16-byte aligned";
    case QUIP_ERR_LAUNCH: return "HIP kernel launch failed";
    case QUIP_ERR_UNSUPPORTED: return "request not supported by this build";
    case QUIP_NO_RESULT: return "measurement launch: the outputs hold no result";
    default: return "unknown quip error";
  }
}

int quip_device_cu_count(void) { return device_cu_count(); }

namespace {
// test helper: `nwg` workgroups that hold `lds` bytes of LDS each (i.e. a CU each above 80 KB) for `ticks` shader clocks
__global__ void occupy_kernel(long long ticks, unsigned* sink) {
  extern __shared__ char smem_occ[];
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  unsigned acc = 0;
  while ((long long)(__builtin_amdgcn_s_memtime() - t0) < ticks) {
    __builtin_amdgcn_s_sleep(32);
    acc += (unsigned)smem_occ[threadIdx.x];
  }
  if (acc == 0x12345678u) *sink = acc;
}
}  // namespace

int quip_debug_occupy(int32_t nwg, int32_t lds_bytes, int64_t ticks, void* sink, quip_stream_t stream) {
  if (nwg < 1 || nwg > 4096 || lds_bytes < 0 || lds_bytes > 160 * 1024 || ticks < 0 || !sink) return QUIP_ERR_BAD_SHAPE;
  return launch<occupy_kernel>(dim3(nwg), dim3(64), lds_bytes, (hipStream_t)stream, (long long)ticks, reinterpret_cast<unsigned*>(sink));
}

namespace {
// ---- the Hadamard transform entry points ---------------------------------------------------------------------------------
// Inside the library a problem is the public quip_had_problem, and every entry ends in had_transform_group_launch
// (hadamard.hip), which answers the sizes, the chain and the optional pointers.  What an entry looks at first is ABI and
// stays its own: had_refusal answers its pointer lists, NULL before MISALIGNED -- the loose-argument entries name x and
// their output (plane images 16-byte aligned), the problem-struct entries every problem's input (x or, chained, z) and
// output, after `problems` and the count.
int had_refusal(Ptrs required, Ptrs a16 = {}) {
  if (any_null(required)) return QUIP_ERR_NULL_POINTER;
  return any_off(a16, 15) ? QUIP_ERR_MISALIGNED : QUIP_OK;
}
int had_group_refusal(const quip_had_problem* problems, int32_t count) {
  if (!problems) return QUIP_ERR_NULL_POINTER;
  if (count < 1 || count > QUIP_MAX_GROUP) return QUIP_ERR_BAD_SHAPE;
  for (int i = 0; i < count; ++i)
    if (int rc = had_refusal({problems[i].x ? problems[i].x : problems[i].z, problems[i].out})) return rc;
  return QUIP_OK;
}
// a loose-argument entry as one problem of the group launcher; planes: one row, out_features = n, no residual
int had_single(bool planes, const void* x, void* out, int64_t rows, int32_t in_features, int32_t out_features, int32_t n,
               int32_t K, const void* had, int32_t transpose, const void* pre_scale, const void* pre_scale2,
               const void* post_scale, const void* bias, float scale, const quip_had_fusion* fusion, quip_stream_t stream) {
  quip_had_problem pr{};
  pr.x = x; pr.out = out; pr.had = had;
  pr.pre_scale = pre_scale; pr.pre_scale2 = pre_scale2; pr.post_scale = post_scale; pr.bias = bias;
  pr.in_features = in_features; pr.out_features = out_features;
  pr.scale = scale; pr.rms_eps = 1e-5f; pr.z_scale = 1.f;
  if (fusion) {
    pr.residual = planes ? nullptr : fusion->residual;
    pr.rms_weight = fusion->rms_weight; pr.gate = fusion->gate; pr.rms_eps = fusion->rms_eps;
  }
  return had_transform_group_launch(&pr, 1, planes, rows, n, K, transpose, (hipStream_t)stream);
}
}  // namespace

int quip_hadamard_f16(const void* x, void* y, int64_t rows, int32_t n, float scale, quip_stream_t stream) {
  if (int rc = had_refusal({x, y})) return rc;
  return had_single(false, x, y, rows, n, n, n, 1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, scale, nullptr, stream);
}

int quip_hadamard(const void* x, void* y, int64_t rows, int32_t n, float scale, int32_t dtype, quip_stream_t stream) {
  if (!x || !y) return QUIP_ERR_NULL_POINTER;
  if (dtype == QUIP_DTYPE_F16) return quip_hadamard_f16(x, y, rows, n, scale, stream);
  return hadamard_generic_launch(x, y, rows, n, scale, dtype, (hipStream_t)stream);
}

int quip_had_transform_f16(const void* x, void* y, int64_t rows, int32_t in_features, int32_t out_features, int32_t n,
                           int32_t K, const void* had, int32_t transpose, const void* pre_scale, const void* pre_scale2,
                           const void* post_scale, const void* bias, float scale, quip_stream_t stream) {
  return quip_had_transform_fused_f16(x, y, rows, in_features, out_features, n, K, had, transpose, pre_scale, pre_scale2,
                                      post_scale, bias, scale, nullptr, stream);
}

int quip_had_transform_planes(const void* x, void* planes, int32_t in_features, int32_t n, int32_t K, const void* had,
                              int32_t transpose, const void* pre_scale, float scale, quip_stream_t stream) {
  return quip_had_transform_planes_fused(x, planes, in_features, n, K, had, transpose, pre_scale, scale, nullptr, stream);
}

int quip_had_transform_fused_f16(const void* x, void* y, int64_t rows, int32_t in_features, int32_t out_features, int32_t n,
                                 int32_t K, const void* had, int32_t transpose, const void* pre_scale, const void* pre_scale2,
                                 const void* post_scale, const void* bias, float scale, const quip_had_fusion* fusion,
                                 quip_stream_t stream) {
  if (int rc = had_refusal({x, y})) return rc;
  return had_single(false, x, y, rows, in_features, out_features, n, K, had, transpose, pre_scale, pre_scale2, post_scale,
                    bias, scale, fusion, stream);
}

int quip_had_transform_planes_fused(const void* x, void* planes, int32_t in_features, int32_t n, int32_t K, const void* had,
                                    int32_t transpose, const void* pre_scale, float scale, const quip_had_fusion* fusion,
                                    quip_stream_t stream) {
  if (int rc = had_refusal({x, planes}, {planes})) return rc;
  return had_single(true, x, planes, 1, in_features, n, n, K, had, transpose, pre_scale, nullptr, nullptr, nullptr, scale,
                    fusion, stream);
}

int quip_had_transform_group_f16(const quip_had_problem* problems, int32_t count, int64_t rows, int32_t n, int32_t K,
                                 int32_t transpose, quip_stream_t stream) {
  if (int rc = had_group_refusal(problems, count)) return rc;
  return had_transform_group_launch(problems, count, false, rows, n, K, transpose, (hipStream_t)stream);
}

int quip_had_transform_planes_group(const quip_had_problem* problems, int32_t count, int32_t n, int32_t K, int32_t transpose,
                                    quip_stream_t stream) {
  if (int rc = had_group_refusal(problems, count)) return rc;
  return had_transform_group_launch(problems, count, true, 1, n, K, transpose, (hipStream_t)stream);
}

int quip_had_transform_planes_rows(const quip_had_problem* problem, int64_t rows, int32_t n, int32_t K,
                                   int32_t transpose, quip_stream_t stream) {
  if (rows < 1) return rows == 0 ? QUIP_OK : QUIP_ERR_BAD_SHAPE;
  if (int rc = had_group_refusal(problem, 1)) return rc;
  return had_transform_group_launch(problem, 1, true, rows, n, K, transpose, (hipStream_t)stream);
}

int quip_had_plan(const quip_had_problem* problems, int32_t count, int32_t planes, int64_t rows, int32_t n, int32_t K,
                  int32_t transpose, int32_t* out) {
  if (!out) return QUIP_ERR_NULL_POINTER;
  for (int i = 0; i < kHadPlanInts; ++i) out[i] = 0;
  out[1] = -1;
  if ((out[0] = had_group_refusal(problems, count)) != QUIP_OK) return out[0];
  return had_transform_group_plan(problems, count, planes != 0, rows, n, K, transpose, device_cu_count(), out);
}
const char* quip_had_plan_kind_name(int32_t kind) { return had_plan_kind_name(kind); }

int quip_e8p_quantize_f32(const void* x, int64_t nvec, const void* grid_packed_abs, void* vals, void* idx,
                          quip_stream_t stream) {
  if (nvec < 0) return QUIP_ERR_BAD_SHAPE;
  if (nvec == 0) return QUIP_OK;
  if (!x || !grid_packed_abs || !vals || !idx) return QUIP_ERR_NULL_POINTER;
  if (!aligned16(x) || !aligned16(vals) || (reinterpret_cast<uintptr_t>(idx) & 7) != 0) return QUIP_ERR_MISALIGNED;
  return e8p_quantize_launch(x, nvec, grid_packed_abs, vals, idx, (hipStream_t)stream);
}

int quip_ldlq_panel_f32(const void* A, const void* B, const void* M, const void* P, int64_t m, int32_t c,
                        const void* grid_packed_abs, void* hat, void* idx, quip_stream_t stream) {
  if (m < 0 || c < 8 || c % 8 != 0) return QUIP_ERR_BAD_SHAPE;
  if (c > 128) return QUIP_ERR_UNSUPPORTED;
  if (m == 0) return QUIP_OK;
  if (!A || !B || !M || !grid_packed_abs || !hat || !idx) return QUIP_ERR_NULL_POINTER;
  if (!aligned16(A) || !aligned16(B) || !aligned16(M) || !aligned16(P) || !aligned16(hat) ||
      (reinterpret_cast<uintptr_t>(idx) & 7) != 0)
    return QUIP_ERR_MISALIGNED;
  return ldlq_panel_launch(A, B, M, P, m, c, grid_packed_abs, hat, idx, (hipStream_t)stream);
}

int quip_ldlq_panel_rvq_f32(const void* A, const void* B, const void* M, const void* P, int64_t m, int32_t c,
                            const void* grid_packed_abs, const void* resid_grid, float resid_scale, void* hat, void* idx,
                            quip_stream_t stream) {
  if (m < 0 || c < 8 || c % 8 != 0) return QUIP_ERR_BAD_SHAPE;
  if (c > 128) return QUIP_ERR_UNSUPPORTED;
  if (!(resid_scale != 0.f) || !(resid_scale - resid_scale == 0.f)) return QUIP_ERR_BAD_SHAPE;     // 0 | nan, +-inf
  if (m == 0) return QUIP_OK;
  if (!A || !B || !M || !grid_packed_abs || !hat || !idx) return QUIP_ERR_NULL_POINTER;
  if (!aligned16(A) || !aligned16(B) || !aligned16(M) || !aligned16(P) || !aligned16(resid_grid) || !aligned16(hat) ||
      (reinterpret_cast<uintptr_t>(idx) & 7) != 0)
    return QUIP_ERR_MISALIGNED;
  return ldlq_panel_rvq_launch(A, B, M, P, m, c, grid_packed_abs, resid_grid, resid_scale, hat, idx, (hipStream_t)stream);
}

int32_t quip_e8p_gemv_max_rows(int32_t n, int32_t k) { return (n > 0 && k > 0) ? e8p_gemv_mfma_max_rows(n, k) : 0; }

int quip_e8p_gemv_planes_rows(const void* planes, const void* qidxs, const void* grid_packed_abs, void* y,
                              int32_t rows, int32_t n, int32_t k, quip_stream_t stream) {
  return quip_gemv_planes_rows_mode(planes, qidxs, grid_packed_abs, nullptr, y, rows, n, k, 0, stream);
}

// rows mode with another table mode: 64 = D4 table (fp16 (256, 4) grid; HI through its virtual layout),
// 40 = E8P12RVQ3B (the 3-byte codes, k = 2 * in features, grid2 = e81b_i8)
int32_t quip_gemv_max_rows_mode(int32_t n, int32_t k, int32_t mode) {
  return (n > 0 && k > 0 && (mode == 0 || mode == 64 || mode == 40)) ? e8p_gemv_mfma_max_rows(n, k, mode) : 0;
}

int quip_gemv_planes_rows_mode(const void* planes, const void* qidxs, const void* grid, const void* grid2, void* y,
                               int32_t rows, int32_t n, int32_t k, int32_t mode, quip_stream_t stream) {
  if (any_null({planes, qidxs, grid, y})) return QUIP_ERR_NULL_POINTER;
  if (rows < 1 || n < 1 || k < 1 || k % 8 != 0) return QUIP_ERR_BAD_SHAPE;
  if (mode != 0 && mode != 64 && mode != 40) return QUIP_ERR_BAD_SHAPE;
  if (mode == 40 && k % 64 != 0) return QUIP_ERR_BAD_SHAPE;   // rows of 3 (k / 2) / 8 bytes, dword aligned
  if (any_off({planes, qidxs}, 15)) return QUIP_ERR_MISALIGNED;
  GemvTune t;
  t.rep = mode;
  t.grid2 = grid2;
  return e8p_gemv_mfma_rows_launch(planes, qidxs, grid, y, rows, n, k, t, (hipStream_t)stream);
}

// 1 = the first kernel, 2 = the K-splitting kernel (either table mode): the first kernel of gemv_plan that takes the shape
int quip_e8p_gemv_kernel_choice(const int32_t* ns, int32_t count, int32_t k) {
  if (!ns) return QUIP_ERR_NULL_POINTER;
  if (count < 1 || count > QUIP_MAX_GROUP || k < 1 || k % 8 != 0) return QUIP_ERR_BAD_SHAPE;
  int n32[QUIP_MAX_GROUP];
  bool v2_ok = true;
  for (int i = 0; i < count; ++i) {
    if (ns[i] < 1) return QUIP_ERR_BAD_SHAPE;
    n32[i] = ns[i];
    v2_ok = v2_ok && e8p_gemv_v2_supported(ns[i], k);
  }
  const GemvPlan plan = gemv_plan(kGemvE8P, n32, count, k);
  for (int i = 0; i < plan.count; ++i) {
    if (plan.kernel[i] == kGemvFirst) return 1;      // (planned only where it takes the shape)
    if (v2_ok) return 2;
  }
  return QUIP_ERR_UNSUPPORTED;
}

size_t quip_e8p_gemv_workspace_bytes(int32_t n_total) {
  return n_total < 1 ? 0 : (e8p_gemv_v2_workspace_words(n_total) + 2 * 64) * 4;
}

int quip_e8p_gemv_planes_group_ws(const void* const* planes, const void* const* qidxs, const void* grid_packed_abs,
                                  void* const* ys, const int32_t* ns, int32_t count, int32_t k, void* workspace,
                                  size_t workspace_bytes, quip_stream_t stream) {
  return gemv_launch(kGemvE8P, planes, qidxs, grid_packed_abs, nullptr, ys, ns, count, k, workspace, workspace_bytes,
                     stream);
}

int quip_e8p_gemv_planes_ws(const void* planes, const void* qidxs, const void* grid, void* y, int32_t n, int32_t k,
                            void* workspace, size_t workspace_bytes, quip_stream_t stream) {
  if (n == 0) return QUIP_OK;
  return gemv_launch(kGemvE8P, &planes, &qidxs, grid, nullptr, &y, &n, 1, k, workspace, workspace_bytes, stream);
}

int quip_e8p_gemv_planes_group(const void* const* planes, const void* const* qidxs,
                               const void* grid_packed_abs, void* const* ys, const int32_t* ns,
                               int32_t count, int32_t k, quip_stream_t stream) {
  return gemv_launch(kGemvE8P, planes, qidxs, grid_packed_abs, nullptr, ys, ns, count, k, nullptr, 0, stream);
}

int quip_e8prvq3_gemv_planes_group(const void* const* planes, const void* const* qidxs,
                                   const void* grid_packed_abs, const void* e81b_i8, void* const* ys,
                                   const int32_t* ns, int32_t count, int32_t k, quip_stream_t stream) {
  return gemv_launch(kGemvRVQ3, planes, qidxs, grid_packed_abs, e81b_i8, ys, ns, count, k, nullptr, 0, stream);
}

int quip_e8prvq3_gemv_planes_group_ws(const void* const* planes, const void* const* qidxs,
                                      const void* grid_packed_abs, const void* e81b_i8, void* const* ys,
                                      const int32_t* ns, int32_t count, int32_t k, void* workspace,
                                      size_t workspace_bytes, quip_stream_t stream) {
  return gemv_launch(kGemvRVQ3, planes, qidxs, grid_packed_abs, e81b_i8, ys, ns, count, k, workspace, workspace_bytes,
                     stream);
}

int quip_d4_gemv_planes(const void* planes, const void* qidxs, const void* grid_f16, void* y, int32_t n,
                        int32_t k, quip_stream_t stream) {
  return gemv_launch(kGemvD4, &planes, &qidxs, grid_f16, nullptr, &y, &n, 1, k, nullptr, 0, stream);
}

int quip_d4_gemv_planes_group(const void* const* planes, const void* const* qidxs, const void* grid_f16,
                              void* const* ys, const int32_t* ns, int32_t count, int32_t k,
                              quip_stream_t stream) {
  return gemv_launch(kGemvD4, planes, qidxs, grid_f16, nullptr, ys, ns, count, k, nullptr, 0, stream);
}

int quip_d4_gemv_planes_v2(const void* planes, const void* qidxs, const void* grid_f16, void* y, int32_t n, int32_t k,
                           void* workspace, size_t workspace_bytes, quip_stream_t stream) {
  // The K-splitting kernel whatever gemv_plan would choose, so not through gemv_launch; its checks are gemv_launch's for
  // one problem in another order -- the shape before the alignment (gemv_launch: per problem the alignment, then n, then
  // k) -- and the table's alignment is the kernel's business.  ABI as recorded; DESIGN 9 item 12.
  if (any_null({planes, qidxs, grid_f16, y})) return QUIP_ERR_NULL_POINTER;
  if (n < 1 || k < 1 || k % kGemvD4.k_multiple != 0) return QUIP_ERR_BAD_SHAPE;
  if (any_off({planes, workspace}, 15) || any_off({qidxs}, kGemvD4.q_mask)) return QUIP_ERR_MISALIGNED;
  if (workspace_bytes < e8p_gemv_v2_workspace_words(n) * 4) workspace = nullptr;
  GemvTune t;
  t.rep = kGemvD4.rep;
  return e8p_gemv_v2_group_launch(&planes, &qidxs, grid_f16, &y, workspace, &n, 1, k, t, (hipStream_t)stream);
}

int quip_d4_gemv_planes_group_ws(const void* const* planes, const void* const* qidxs, const void* grid_f16,
                                 void* const* ys, const int32_t* ns, int32_t count, int32_t k, void* workspace,
                                 size_t workspace_bytes, quip_stream_t stream) {
  return gemv_launch(kGemvD4, planes, qidxs, grid_f16, nullptr, ys, ns, count, k, workspace, workspace_bytes, stream);
}

int quip_e8p_gemv_fused(const quip_gemv_fused_in* in, const void* const* qidxs,
                        const void* grid_packed_abs, void* const* ys, const int32_t* ns,
                        int32_t count, int32_t k, quip_stream_t stream) {
  if (!in || !qidxs || !grid_packed_abs || !ys || !ns) return QUIP_ERR_NULL_POINTER;
  if (count < 1 || count > QUIP_MAX_GROUP) return QUIP_ERR_BAD_SHAPE;
  const GemvFusedIn f = fused_in_of(in, count);
  if (!f.z && !f.x) return QUIP_ERR_NULL_POINTER;
  if (f.z && (!f.post || !f.h_out)) return QUIP_ERR_NULL_POINTER;
  if (f.z && f.h_out == f.residual) return QUIP_ERR_BAD_SHAPE;
  if (any_off({f.x, f.z, f.post, f.residual, f.h_out, f.rms_w}, 15)) return QUIP_ERR_MISALIGNED;
  int n32[QUIP_MAX_GROUP];
  for (int i = 0; i < count; ++i) {
    if (any_null({qidxs[i], ys[i], f.pre[i]})) return QUIP_ERR_NULL_POINTER;
    if (any_off({qidxs[i], f.pre[i]}, 15)) return QUIP_ERR_MISALIGNED;
    if (ns[i] < 1) return QUIP_ERR_BAD_SHAPE;
    n32[i] = ns[i];
  }
  return e8p_gemv_mfma_fused_launch(f, qidxs, grid_packed_abs, ys, n32, count, k, GemvTune{}, (hipStream_t)stream);
}

int quip_argmax_step_f16(const void* logits, int32_t n, void* tok, void* pos, quip_stream_t stream) {
  if (!logits || !tok || !pos) return QUIP_ERR_NULL_POINTER;
  if (!aligned16(logits) || (reinterpret_cast<uintptr_t>(tok) & 7) || (reinterpret_cast<uintptr_t>(pos) & 7))
    return QUIP_ERR_MISALIGNED;
  return argmax_step_launch(logits, n, tok, pos, (hipStream_t)stream);
}

int quip_ffn_engine_supported(int32_t hidden, int32_t n_ffn, int32_t K) {
  return ffn_engine_supported(hidden, n_ffn, K) ? 1 : 0;
}

size_t quip_ffn_engine_workspace_bytes(int32_t n_ffn, int32_t K) {
  return (n_ffn > 0 && K > 0 && n_ffn % K == 0) ? ffn_engine_workspace_bytes(n_ffn, K) : 0;
}

int quip_ffn_engine(const quip_ffn_engine_args* in, quip_stream_t stream) {
  if (!in) return QUIP_ERR_NULL_POINTER;
  if (!in->w_gate || !in->w_up || !in->w_down || !in->planes_gate || !in->planes_up || !in->had3 || !in->sv_gate ||
      !in->sv_up || !in->su_down || !in->z_down || !in->grid_packed_abs || !in->workspace)
    return QUIP_ERR_NULL_POINTER;
  if (!aligned16(in->w_gate) || !aligned16(in->w_up) || !aligned16(in->w_down) || !aligned16(in->planes_gate) ||
      !aligned16(in->planes_up) || !aligned16(in->had3) || !aligned16(in->sv_gate) || !aligned16(in->sv_up) ||
      !aligned16(in->su_down) || !aligned16(in->workspace) || (reinterpret_cast<uintptr_t>(in->grid_packed_abs) & 63u) != 0)
    return QUIP_ERR_MISALIGNED;
  if (in->hidden < 1 || in->n_ffn < 1 || in->K < 1) return QUIP_ERR_BAD_SHAPE;
  FfnEngineArgs a;
  a.w_gate = in->w_gate; a.w_up = in->w_up; a.w_down = in->w_down;
  a.planes_gate = in->planes_gate; a.planes_up = in->planes_up; a.had3 = in->had3;
  a.sv_gate = in->sv_gate; a.sv_up = in->sv_up; a.su_down = in->su_down;
  a.z_down = in->z_down; a.grid = in->grid_packed_abs; a.workspace = in->workspace; a.dbg = in->dbg;
  a.out_scale = in->out_scale; a.in_scale = in->in_scale;
  a.hidden = in->hidden; a.n_ffn = in->n_ffn; a.K = in->K;
  return ffn_engine_launch(a, (hipStream_t)stream);
}

int quip_block_engine_supported(int32_t hidden, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t n_ffn, int32_t K) {
  return block_engine_supported(hidden, heads, kv_heads, head_dim, n_ffn, K) ? 1 : 0;
}

size_t quip_block_engine_workspace_bytes(void) { return block_engine_workspace_bytes(); }
size_t quip_block_engine_layer_bytes(void) { return block_engine_layer_bytes(); }

namespace {
// the public arguments (and, for a whole-token launch, its tail `t`: h_in is then the embedding row of *t->tok) as
// BlockEngineArgs; codebook 4 needs its second table, 8-byte aligned
int block_engine_args_of(const quip_block_engine_args* in, const quip_token_tail_args* t, BlockEngineArgs& a) {
  a.layers = in->layers; a.h_in = t ? nullptr : in->h_in; a.h_out = in->h_out; a.pos = in->pos; a.cos = in->cos; a.sin = in->sin;
  a.grid = in->grid_packed_abs; a.workspace = in->workspace; a.dbg = in->dbg;
  a.n_layers = in->n_layers; a.max_len = in->max_len; a.dbg_layer = in->dbg_layer;
  a.rms_eps = in->rms_eps; a.attn_scale = in->attn_scale; a.codebook = in->codebook; a.resid_scale = in->resid_scale;
  a.grid2 = in->grid2;
  if (in->codebook == 4 && (!in->grid2 || (reinterpret_cast<uintptr_t>(in->grid2) & 7u) != 0))
    return in->grid2 ? QUIP_ERR_MISALIGNED : QUIP_ERR_NULL_POINTER;
  if (t) {
    a.tok = t->tok; a.embed = t->embed; a.final_norm = t->final_norm; a.lm_head = t->lm_head; a.logits = t->logits;
    a.xnorm = t->xnorm; a.vocab = t->vocab;
  }
  return QUIP_OK;
}
}  // namespace

int quip_block_engine(const quip_block_engine_args* in, quip_stream_t stream) {
  if (!in) return QUIP_ERR_NULL_POINTER;
  if (!in->layers || !in->h_in || !in->h_out || !in->pos || !in->cos || !in->sin || !in->grid_packed_abs || !in->workspace)
    return QUIP_ERR_NULL_POINTER;
  if (!aligned16(in->layers) || !aligned16(in->h_in) || !aligned16(in->h_out) || !aligned16(in->workspace) ||
      (reinterpret_cast<uintptr_t>(in->grid_packed_abs) & 63u) != 0)
    return QUIP_ERR_MISALIGNED;
  if (in->n_layers < 1 || in->max_len < 1) return QUIP_ERR_BAD_SHAPE;
  BlockEngineArgs a;
  if (const int rc = block_engine_args_of(in, nullptr, a); rc != QUIP_OK) return rc;
  if (in->shape == 1) return block_engine_gqa_launch(a, (hipStream_t)stream);
  if (in->shape == 2) return block_engine_g8_launch(a, (hipStream_t)stream);
  if (in->shape != 0) return QUIP_ERR_UNSUPPORTED;
  return block_engine_launch(a, (hipStream_t)stream);
}

int quip_block_engine_token(const quip_block_engine_args* in, const quip_token_tail_args* t, quip_stream_t stream) {
  if (!in || !t) return QUIP_ERR_NULL_POINTER;
  if (!in->layers || !in->pos || !in->cos || !in->sin || !in->grid_packed_abs || !in->workspace || !t->tok || !t->pos ||
      !t->embed || !t->final_norm || !t->lm_head || !t->logits)
    return QUIP_ERR_NULL_POINTER;
  if (!aligned16(in->layers) || !aligned16(in->workspace) || (in->h_out && !aligned16(in->h_out)) ||
      (reinterpret_cast<uintptr_t>(in->grid_packed_abs) & 63u) != 0 || !aligned16(t->embed) || !aligned16(t->lm_head) ||
      !aligned16(t->logits) || !aligned16(t->final_norm) || (t->xnorm && !aligned16(t->xnorm)) ||
      (reinterpret_cast<uintptr_t>(t->tok) & 7u) != 0 || (reinterpret_cast<uintptr_t>(t->pos) & 7u) != 0)
    return QUIP_ERR_MISALIGNED;
  if (in->n_layers < 1 || in->max_len < 1 || t->vocab < 256 || t->vocab >= 256 * 65535) return QUIP_ERR_BAD_SHAPE;
  if (t->pos != in->pos) return QUIP_ERR_BAD_SHAPE;              // ONE position counter: read at the top, advanced at the end
  if (in->shape != 0 && in->shape != 2) return QUIP_ERR_UNSUPPORTED;
  BlockEngineArgs a;
  if (const int rc = block_engine_args_of(in, t, a); rc != QUIP_OK) return rc;
  if (in->shape == 2) return block_engine_g8_launch(a, (hipStream_t)stream);
  return block_engine_launch(a, (hipStream_t)stream);
}

namespace {
// tiled[rb][c][q][n] = bytes [64 c + 16 q, +16) of row 16 rb + n: one 16-byte piece per thread, destination order
__global__ void tile_codes_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, long long pieces, int row_u4) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pieces) return;
  const int n = (int)(i & 15), q = (int)((i >> 4) & 3);
  const long long cc = i >> 6;                         // (row block, 64-byte piece) pairs
  const int pieces_per_row = row_u4 / 4;
  const long long rb = cc / pieces_per_row;
  const int c = (int)(cc - rb * pieces_per_row);
  dst[i] = src[(rb * 16 + n) * row_u4 + c * 4 + q];
}
// the inverse: piece i of the tiled copy back to its place in the row-major matrix
__global__ void untile_codes_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, long long pieces, int row_u4) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pieces) return;
  const int n = (int)(i & 15), q = (int)((i >> 4) & 3);
  const long long cc = i >> 6;
  const int pieces_per_row = row_u4 / 4;
  const long long rb = cc / pieces_per_row;
  const int c = (int)(cc - rb * pieces_per_row);
  dst[(rb * 16 + n) * row_u4 + c * 4 + q] = src[i];
}

// src -> dst through tile_codes_kernel or its inverse, one 16-byte piece per thread
int retile_codes(bool inverse, const void* src, void* dst, int64_t rows, int64_t row_bytes, quip_stream_t stream) {
  if (!src || !dst) return QUIP_ERR_NULL_POINTER;
  if (rows < 0 || row_bytes <= 0 || rows % 16 != 0 || row_bytes % 64 != 0 || row_bytes > (1 << 24)) return QUIP_ERR_BAD_SHAPE;
  if (rows == 0) return QUIP_OK;
  if (!aligned16(src) || !aligned16(dst)) return QUIP_ERR_MISALIGNED;
  {
    // not in place, and no partial overlap either: the kernel gathers from the source while it scatters
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t bytes = (uintptr_t)rows * (uintptr_t)row_bytes;
    if (s0 < d0 + bytes && d0 < s0 + bytes) return QUIP_ERR_UNSUPPORTED;
  }
  const long long pieces = rows * (row_bytes / 16);
  const dim3 grid((unsigned)((pieces + 255) / 256)), block(256);
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  return inverse ? launch<untile_codes_kernel>(grid, block, 0, (hipStream_t)stream, s, d, pieces, (int)(row_bytes / 16))
                 : launch<tile_codes_kernel>(grid, block, 0, (hipStream_t)stream, s, d, pieces, (int)(row_bytes / 16));
}

// The (K, 256) view of a gate / up matrix (rows k * 256 + j: column j of the view), column by column, in blocks of 16 view rows, the
// last one short, without padding: view[j][b][c][q][n < nb(b)] = bytes [64 c + 16 q, +16) of row (16 b + n) * 256 + j.  One 16-byte
// piece per thread, in the order of the tiled side; `inverse` scatters it back.
__global__ void tile_codes_view_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, long long pieces, int row_u4, int K, int inverse) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pieces) return;
  const int col_u4 = K * row_u4;                       // pieces of a column: K rows
  const int j = (int)(i / col_u4);
  int r = (int)(i - (long long)j * col_u4);
  const int b = r / (16 * row_u4);                     // (the blocks in front of a block are full ones)
  r -= b * 16 * row_u4;
  const int nb = K - 16 * b < 16 ? K - 16 * b : 16;
  const int c = r / (4 * nb);
  r -= c * 4 * nb;
  const int q = r / nb, n = r - q * nb;
  const long long rm = ((long long)(16 * b + n) * 256 + j) * row_u4 + c * 4 + q;
  if (inverse) dst[rm] = src[i];
  else dst[i] = src[rm];
}

int retile_codes_view(bool inverse, const void* src, void* dst, int64_t rows, int64_t row_bytes, quip_stream_t stream) {
  if (!src || !dst) return QUIP_ERR_NULL_POINTER;
  if (rows < 0 || row_bytes <= 0 || rows % 256 != 0 || row_bytes % 64 != 0 || row_bytes > (1 << 24) || rows > (1 << 24))
    return QUIP_ERR_BAD_SHAPE;
  if (rows == 0) return QUIP_OK;
  if (!aligned16(src) || !aligned16(dst)) return QUIP_ERR_MISALIGNED;
  {
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t bytes = (uintptr_t)rows * (uintptr_t)row_bytes;
    if (s0 < d0 + bytes && d0 < s0 + bytes) return QUIP_ERR_UNSUPPORTED;
  }
  const long long pieces = rows * (row_bytes / 16);
  if ((rows / 256) * (row_bytes / 16) > (1ll << 30)) return QUIP_ERR_BAD_SHAPE;      // (a column's pieces: int arithmetic in the kernel)
  const dim3 grid((unsigned)((pieces + 255) / 256)), block(256);
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  const int row_u4 = (int)(row_bytes / 16), K = (int)(rows / 256);
  return launch<tile_codes_view_kernel>(grid, block, 0, (hipStream_t)stream, s, d, pieces, row_u4, K, inverse ? 1 : 0);
}
}  // namespace

int quip_tile_codes_view(const void* qidxs, void* tiled, int64_t rows, int64_t row_bytes, quip_stream_t stream) {
  return retile_codes_view(false, qidxs, tiled, rows, row_bytes, stream);
}

int quip_untile_codes_view(const void* tiled, void* qidxs, int64_t rows, int64_t row_bytes, quip_stream_t stream) {
  return retile_codes_view(true, tiled, qidxs, rows, row_bytes, stream);
}

int quip_tile_codes(const void* qidxs, void* tiled, int64_t rows, int64_t row_bytes, quip_stream_t stream) {
  return retile_codes(false, qidxs, tiled, rows, row_bytes, stream);
}

int quip_untile_codes(const void* tiled, void* qidxs, int64_t rows, int64_t row_bytes, quip_stream_t stream) {
  return retile_codes(true, tiled, qidxs, rows, row_bytes, stream);
}

int quip_block_engine_gqa_supported(int32_t hidden, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t n_ffn, int32_t K) {
  return block_engine_gqa_supported(hidden, heads, kv_heads, head_dim, n_ffn, K) ? 1 : 0;
}
size_t quip_block_engine_gqa_workspace_bytes(void) { return block_engine_gqa_workspace_bytes(); }
int quip_block_engine_g8_supported(int32_t hidden, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t n_ffn, int32_t K) {
  return block_engine_g8_supported(hidden, heads, kv_heads, head_dim, n_ffn, K) ? 1 : 0;
}
size_t quip_block_engine_g8_workspace_bytes(void) { return block_engine_g8_workspace_bytes(); }

// ---- the attention entry points ------------------------------------------------------------------------------------------
// Each one is its own pointer lists and one call.  attn_refusal answers what is wrong with the pointers and the window in
// the order the ABI promises: NULL (the nine operands of AttnIO and `more`), then MISALIGNED (the 16-, 8- and 4-byte lists;
// the optional workspace: 16), then a negative window (BAD_SHAPE).  The launcher (quip_internal.h) answers the sizes,
// BAD_SHAPE before UNSUPPORTED.  The lists differ from entry to entry and are part of the ABI as they are: the bs = 1
// entries do not look at the alignment of pos, only the prompt-side entries at that of out / cos / sin, and those leave
// the window to their launcher.
namespace {
int attn_refusal(const AttnIO& io, Ptrs more, Ptrs a16, Ptrs a8 = {}, Ptrs a4 = {}, const void* workspace = nullptr,
                 int window = 0) {
  if (any_null({io.q, io.k, io.v, io.cos, io.sin, io.pos, io.kcache, io.vcache, io.out}) || any_null(more))
    return QUIP_ERR_NULL_POINTER;
  if (any_off(a16, 15) || any_off(a8, 7) || any_off(a4, 3) || any_off({workspace}, 15)) return QUIP_ERR_MISALIGNED;
  return window < 0 ? QUIP_ERR_BAD_SHAPE : QUIP_OK;
}
}  // namespace

size_t quip_rope_attn_workspace_bytes(int32_t heads, int32_t head_dim) {
  return heads > 0 && head_dim > 0 ? rope_attn_workspace_bytes(heads, head_dim) : 0;
}

int quip_rope_attn_decode_f16(const void* q, const void* k, const void* v, const float* cos,
                              const float* sin, const int64_t* pos, void* kcache, void* vcache,
                              void* out, int32_t heads, int32_t kv_heads, int32_t head_dim,
                              int32_t max_len, float scale, void* workspace, quip_stream_t stream) {
  return quip_rope_attn_decode_window_f16(q, k, v, cos, sin, pos, kcache, vcache, out, heads, kv_heads, head_dim, max_len,
                                          scale, 0, workspace, stream);
}

int quip_rope_attn_decode_window_f16(const void* q, const void* k, const void* v, const float* cos,
                                     const float* sin, const int64_t* pos, void* kcache, void* vcache,
                                     void* out, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                     int32_t max_len, float scale, int32_t window, void* workspace,
                                     quip_stream_t stream) {
  const AttnIO io{q, k, v, cos, sin, pos, kcache, vcache, out};
  const AttnShape s{1, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {}, {q, k, v, kcache, vcache}, {}, {}, workspace, window)) return rc;
  return rope_attn_decode_launch(io, s, (hipStream_t)stream, workspace);
}

size_t quip_rope_attn_batched_workspace_bytes(int32_t batch, int32_t heads, int32_t head_dim) {
  return batch > 0 && heads > 0 && head_dim > 0 ? rope_attn_batched_workspace_bytes(batch, heads, head_dim) : 0;
}

int quip_rope_attn_decode_batched_f16(const void* q, const void* k, const void* v, const float* cos,
                                      const float* sin, const int64_t* pos, void* kcache, void* vcache,
                                      void* out, int32_t batch, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                      int32_t max_len, float scale, int32_t window, void* workspace,
                                      quip_stream_t stream) {
  const AttnIO io{q, k, v, cos, sin, pos, kcache, vcache, out};
  const AttnShape s{batch, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {}, {q, k, v, kcache, vcache}, {pos}, {}, workspace, window)) return rc;
  return rope_attn_decode_batched_launch(io, s, (hipStream_t)stream, workspace);
}

int quip_rope_attn_decode_batched_start_f16(const void* q, const void* k, const void* v, const float* cos,
                                            const float* sin, const int64_t* pos, void* kcache, void* vcache,
                                            void* out, int32_t batch, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                            int32_t max_len, float scale, int32_t window, void* workspace,
                                            quip_stream_t stream, const void* start) {
  const AttnIO io{q, k, v, cos, sin, pos, kcache, vcache, out};
  const AttnShape s{batch, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {start}, {q, k, v, kcache, vcache}, {pos, start}, {}, workspace, window)) return rc;
  return rope_attn_decode_batched_start_launch(io, reinterpret_cast<const int64_t*>(start), s, (hipStream_t)stream,
                                               workspace);
}

int quip_rope_attn_chunk_f16(const void* q, const void* k, const void* v, const float* cos, const float* sin,
                             const int64_t* pos, void* kcache, void* vcache, void* out, int32_t rows, int32_t heads,
                             int32_t kv_heads, int32_t head_dim, int32_t max_len, float scale, int32_t window,
                             quip_stream_t stream) {
  const AttnIO io{q, k, v, cos, sin, pos, kcache, vcache, out};
  const AttnShape s{1, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {}, {q, k, v, kcache, vcache, out, cos, sin}, {pos})) return rc;
  return rope_attn_chunk_launch(io, s, rows, (hipStream_t)stream);
}

int quip_rope_attn_ragged_f16(const void* q, const void* k, const void* v, const float* cos, const float* sin,
                              const int64_t* pos, void* kcache, void* vcache, void* out, int32_t rows, int32_t heads,
                              int32_t kv_heads, int32_t head_dim, int32_t max_len, int32_t batch,
                              const int32_t* seg_slot, const int32_t* seg_rows, int32_t nseg, float scale,
                              int32_t window, quip_stream_t stream) {
  const AttnIO io{q, k, v, cos, sin, pos, kcache, vcache, out};
  const AttnShape s{batch, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {seg_slot, seg_rows}, {q, k, v, kcache, vcache, out, cos, sin}, {pos})) return rc;
  return rope_attn_ragged_launch(io, s, rows, {seg_slot, seg_rows, nseg}, (hipStream_t)stream);
}

int quip_rope_attn_decode_paged_f16(const void* q, const void* k, const void* v, const float* cos, const float* sin,
                                    const int64_t* pos, const int32_t* table, void* kpool, void* vpool, void* out,
                                    int32_t batch, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t max_len,
                                    int32_t n_pages, int32_t max_pages, float scale, int32_t window, void* workspace,
                                    quip_stream_t stream) {
  const AttnIO io{q, k, v, cos, sin, pos, kpool, vpool, out};
  const AttnShape s{batch, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {table}, {q, k, v, kpool, vpool}, {pos}, {table}, workspace, window)) return rc;
  return rope_attn_decode_paged_launch(io, {table, n_pages, max_pages, 0, 0}, s, (hipStream_t)stream, workspace);
}

int quip_rope_attn_ragged_paged_f16(const void* q, const void* k, const void* v, const float* cos, const float* sin,
                                    const int64_t* pos, const int32_t* table, void* kpool, void* vpool, void* out,
                                    int32_t rows, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t max_len,
                                    int32_t batch, int32_t n_pages, int32_t max_pages, const int32_t* seg_slot,
                                    const int32_t* seg_rows, int32_t nseg, float scale, int32_t window,
                                    quip_stream_t stream) {
  const AttnIO io{q, k, v, cos, sin, pos, kpool, vpool, out};
  const AttnShape s{batch, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {table, seg_slot, seg_rows}, {q, k, v, kpool, vpool, out, cos, sin}, {pos}, {table})) return rc;
  return rope_attn_ragged_paged_launch(io, {table, n_pages, max_pages, 0, 0}, s, rows, {seg_slot, seg_rows, nseg},
                                       (hipStream_t)stream);
}

int quip_rope_attn_decode_paged_f8(const void* q, const void* k, const void* v, const float* cos, const float* sin,
                                   const int64_t* pos, const int32_t* table, void* kpool, void* vpool, void* out,
                                   int32_t batch, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t max_len,
                                   int32_t n_pages, int32_t max_pages, float scale, int32_t window, void* workspace,
                                   quip_stream_t stream, int32_t k_exp, int32_t v_exp) {
  const AttnIO io{q, k, v, cos, sin, pos, kpool, vpool, out};
  const AttnShape s{batch, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {table}, {q, k, v, kpool, vpool}, {pos}, {table}, workspace, window)) return rc;
  return rope_attn_decode_paged_f8_launch(io, {table, n_pages, max_pages, k_exp, v_exp}, s, (hipStream_t)stream, workspace);
}

int quip_rope_attn_ragged_paged_f8(const void* q, const void* k, const void* v, const float* cos, const float* sin,
                                   const int64_t* pos, const int32_t* table, void* kpool, void* vpool, void* out,
                                   int32_t rows, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t max_len,
                                   int32_t batch, int32_t n_pages, int32_t max_pages, const int32_t* seg_slot,
                                   const int32_t* seg_rows, int32_t nseg, float scale, int32_t window,
                                   quip_stream_t stream, int32_t k_exp, int32_t v_exp) {
  const AttnIO io{q, k, v, cos, sin, pos, kpool, vpool, out};
  const AttnShape s{batch, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {table, seg_slot, seg_rows}, {q, k, v, kpool, vpool, out, cos, sin}, {pos}, {table})) return rc;
  return rope_attn_ragged_paged_f8_launch(io, {table, n_pages, max_pages, k_exp, v_exp}, s, rows, {seg_slot, seg_rows, nseg},
                                          (hipStream_t)stream);
}

int quip_argmax_step_batched_f16(const void* logits, int32_t batch, int32_t n, void* tok, void* pos,
                                 quip_stream_t stream) {
  if (!logits || !tok || !pos) return QUIP_ERR_NULL_POINTER;
  if (!aligned16(logits) || (reinterpret_cast<uintptr_t>(tok) & 7) || (reinterpret_cast<uintptr_t>(pos) & 7))
    return QUIP_ERR_MISALIGNED;
  return argmax_step_batched_launch(logits, batch, n, tok, pos, (hipStream_t)stream);
}

int quip_nll_rows_f16(const void* logits, int32_t rows, int32_t n, const int64_t* target, float* logprob, float* lse,
                      int64_t* argmax, quip_stream_t stream) {
  if (!logits || !target || !logprob) return QUIP_ERR_NULL_POINTER;
  if ((reinterpret_cast<uintptr_t>(logits) & 1) || (reinterpret_cast<uintptr_t>(target) & 7) ||
      (reinterpret_cast<uintptr_t>(logprob) & 3) || (reinterpret_cast<uintptr_t>(lse) & 3) ||
      (reinterpret_cast<uintptr_t>(argmax) & 7))
    return QUIP_ERR_MISALIGNED;
  return nll_rows_launch(logits, rows, n, target, logprob, lse, argmax, (hipStream_t)stream);
}

int quip_sample_step_f16(const void* logits, int32_t rows, int32_t n, const float* temperature, const int32_t* top_k,
                         const float* top_p, const int64_t* seed, int64_t* tok, int64_t* pos, int32_t* kept,
                         quip_stream_t stream) {
  if (!logits || !temperature || !top_k || !top_p || !seed || !tok || !pos) return QUIP_ERR_NULL_POINTER;
  if ((reinterpret_cast<uintptr_t>(logits) & 1) || (reinterpret_cast<uintptr_t>(temperature) & 3) ||
      (reinterpret_cast<uintptr_t>(top_k) & 3) || (reinterpret_cast<uintptr_t>(top_p) & 3) ||
      (reinterpret_cast<uintptr_t>(seed) & 7) || (reinterpret_cast<uintptr_t>(tok) & 7) ||
      (reinterpret_cast<uintptr_t>(pos) & 7) || (reinterpret_cast<uintptr_t>(kept) & 3))
    return QUIP_ERR_MISALIGNED;
  return sample_rows_launch(logits, rows, n, temperature, top_k, top_p, seed, tok, pos, kept, (hipStream_t)stream);
}

int quip_spec_draft_i64(int64_t* rows_tok, int32_t* n_draft, int64_t* pos, int64_t* hist, int32_t hist_cap,
                        const int64_t* pred, const int32_t* n_pred, int32_t pred_cap, int64_t* stats, int32_t k,
                        int32_t gmin, int32_t gmax, quip_stream_t stream) {
  if (any_null({rows_tok, n_draft, pos, hist, n_pred, stats}) || (!pred && pred_cap != 0)) return QUIP_ERR_NULL_POINTER;
  if (any_off({rows_tok, pos, hist, pred, stats}, 7) || any_off({n_draft, n_pred}, 3)) return QUIP_ERR_MISALIGNED;
  return spec_draft_launch(rows_tok, n_draft, pos, hist, hist_cap, pred, n_pred, pred_cap, stats, k, gmin, gmax,
                           (hipStream_t)stream);
}

int quip_spec_accept_draft_i64(const int64_t* argmax, const float* lse, int64_t* rows_tok, int32_t* n_draft, int64_t* pos,
                               int64_t* hist, int32_t hist_cap, const int64_t* pred, const int32_t* n_pred,
                               int32_t pred_cap, int64_t* out, int64_t* out_len, int32_t cap_out, int64_t* stats,
                               int32_t k, int32_t gmin, int32_t gmax, quip_stream_t stream) {
  if (any_null({argmax, lse, rows_tok, n_draft, pos, hist, n_pred, out_len, stats}) || (!pred && pred_cap != 0) ||
      (!out && cap_out != 0))
    return QUIP_ERR_NULL_POINTER;
  if (any_off({argmax, rows_tok, pos, hist, pred, out, out_len, stats}, 7) || any_off({lse, n_draft, n_pred}, 3))
    return QUIP_ERR_MISALIGNED;
  return spec_accept_draft_launch(argmax, lse, rows_tok, n_draft, pos, hist, hist_cap, pred, n_pred, pred_cap, out, out_len,
                                  cap_out, stats, k, gmin, gmax, (hipStream_t)stream);
}

int quip_qk_norm_rows_f16(void* q, void* k, const void* q_weight, const void* k_weight, int64_t rows, int32_t heads,
                          int32_t kv_heads, int32_t head_dim, float eps, quip_stream_t stream) {
  if (any_null({q, k, q_weight, k_weight})) return QUIP_ERR_NULL_POINTER;
  if (any_off({q, k, q_weight, k_weight}, 15)) return QUIP_ERR_MISALIGNED;
  return qk_norm_rows_launch(q, k, q_weight, k_weight, rows, heads, kv_heads, head_dim, eps, (hipStream_t)stream);
}

int quip_rope_attn_decode_qknorm_f16(const void* q, const void* k, const void* v, const float* cos, const float* sin,
                                     const int64_t* pos, void* kcache, void* vcache, void* out, int32_t heads,
                                     int32_t kv_heads, int32_t head_dim, int32_t max_len, float scale, int32_t window,
                                     void* workspace, quip_stream_t stream, const void* q_weight, const void* k_weight,
                                     float eps) {
  const AttnIO io{q, k, v, cos, sin, pos, kcache, vcache, out};
  const AttnShape s{1, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {q_weight, k_weight}, {q, k, v, kcache, vcache, q_weight, k_weight}, {}, {}, workspace, window))
    return rc;
  return rope_attn_decode_qknorm_launch(io, s, {q_weight, k_weight, eps}, (hipStream_t)stream, workspace);
}

int quip_rope_attn_decode_batched_qknorm_f16(const void* q, const void* k, const void* v, const float* cos,
                                             const float* sin, const int64_t* pos, void* kcache, void* vcache, void* out,
                                             int32_t batch, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                             int32_t max_len, float scale, int32_t window, void* workspace,
                                             quip_stream_t stream, const void* q_weight, const void* k_weight, float eps) {
  const AttnIO io{q, k, v, cos, sin, pos, kcache, vcache, out};
  const AttnShape s{batch, heads, kv_heads, head_dim, max_len, window, scale};
  if (int rc = attn_refusal(io, {q_weight, k_weight}, {q, k, v, kcache, vcache, q_weight, k_weight}, {pos}, {}, workspace, window))
    return rc;
  return rope_attn_decode_batched_qknorm_launch(io, s, {q_weight, k_weight, eps}, (hipStream_t)stream, workspace);
}

int quip_lora_shrink_rows_f16(const void* x, const void* A, const int32_t* row_adapter, float* t, int64_t rows, int32_t in,
                              int32_t R, int32_t n_adapters, int32_t mode, const void* aux, float eps, quip_stream_t stream) {
  if (!x || !A || !row_adapter || !t || (mode != 0 && !aux)) return QUIP_ERR_NULL_POINTER;
  if (!aligned16(x) || !aligned16(A) || (mode != 0 && !aligned16(aux)) || (reinterpret_cast<uintptr_t>(row_adapter) & 3) ||
      (reinterpret_cast<uintptr_t>(t) & 3))
    return QUIP_ERR_MISALIGNED;
  return lora_shrink_rows_launch(x, A, row_adapter, t, rows, in, R, n_adapters, mode, aux, eps, (hipStream_t)stream);
}

int quip_lora_expand_rows_f16(const float* t, const int32_t* row_adapter, const float* scale, int64_t rows, int32_t R_total,
                              int32_t n_adapters, int32_t segments, void* const* y, const void* const* B, const int32_t* out,
                              const int32_t* R, const int32_t* r0, quip_stream_t stream) {
  if (!t || !row_adapter || !scale || !y || !B || !out || !R || !r0) return QUIP_ERR_NULL_POINTER;
  if ((reinterpret_cast<uintptr_t>(t) & 3) || (reinterpret_cast<uintptr_t>(row_adapter) & 3) ||
      (reinterpret_cast<uintptr_t>(scale) & 3))
    return QUIP_ERR_MISALIGNED;
  return lora_expand_rows_launch(t, row_adapter, scale, rows, R_total, n_adapters, segments, y, B, out, R, r0,
                                 (hipStream_t)stream);
}

int quip_rope_attn_decode_z_supported(int32_t heads, int32_t kv_heads, int32_t head_dim) {
  return rope_attn_decode_z_supported(heads, kv_heads, head_dim) ? 1 : 0;
}

int quip_rope_attn_decode_z_f16(const void* const* z, const void* const* post, const float* scales, const float* cos,
                                const float* sin, const int64_t* pos, void* kcache, void* vcache, void* out,
                                int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t max_len, float scale,
                                void* workspace, quip_stream_t stream) {
  return quip_rope_attn_decode_z_window_f16(z, post, scales, cos, sin, pos, kcache, vcache, out, heads, kv_heads, head_dim,
                                            max_len, scale, 0, workspace, stream);
}

int quip_rope_attn_decode_z_window_f16(const void* const* z, const void* const* post, const float* scales,
                                       const float* cos, const float* sin, const int64_t* pos, void* kcache, void* vcache,
                                       void* out, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t max_len,
                                       float scale, int32_t window, void* workspace, quip_stream_t stream) {
  if (any_null({z, post, scales, cos, sin, pos, kcache, vcache, out})) return QUIP_ERR_NULL_POINTER;
  for (int i = 0; i < 3; ++i) {     // (element by element: a misaligned z[0] is answered before a NULL z[1])
    if (any_null({z[i], post[i]})) return QUIP_ERR_NULL_POINTER;
    if (any_off({z[i], post[i]}, 15)) return QUIP_ERR_MISALIGNED;
  }
  if (any_off({kcache, vcache, workspace}, 15)) return QUIP_ERR_MISALIGNED;
  if (window < 0) return QUIP_ERR_BAD_SHAPE;
  return rope_attn_decode_z_launch(z, post, scales, {nullptr, nullptr, nullptr, cos, sin, pos, kcache, vcache, out},
                                   {1, heads, kv_heads, head_dim, max_len, window, scale}, (hipStream_t)stream, workspace);
}

// ---- the products: an entry is its argument list, its CodebookArgs and one call of its family ---------------------------
// E8P12 has two fast paths above the original-order family: one row on the VALU integer GEMV, and (_ws) fewer than 32 rows
// through digit planes and rows mode on the matrix cores.  Either is taken only where every argument it needs is there and
// aligned; everything else, and every refusal, is the family's.
int quip_e8p_mm_origorder(const void* x, const void* qidxs, const void* grid, void* y, int32_t m,
                          int32_t n, int32_t k, quip_stream_t stream) {
  if (!any_null({grid, x, qidxs, y}) && m == 1 && n > 0 && e8p_gemv_i8_supported(n, k) && !any_off({x, qidxs}, 15))
    return e8p_gemv_i8_launch(x, 1, qidxs, grid, y, n, k, GemvTune{}, (hipStream_t)stream);
  return mm_origorder(kE8P, x, qidxs, {grid}, y, m, n, k, stream);
}

size_t quip_e8p_planes_bytes(int32_t k) { return k > 0 ? e8p_gemv_mfma_planes_bytes(k) : 0; }

size_t quip_e8p_mm_workspace_bytes(int32_t m, int32_t n, int32_t k) {
  return (m >= 1 && m < 32 && e8p_gemv_mfma_supported(n, k)) ? (size_t)m * e8p_gemv_mfma_planes_bytes(k) : 0;
}

int quip_e8p_x_to_planes(const void* x, void* planes, int32_t k, quip_stream_t stream) {
  if (any_null({x, planes})) return QUIP_ERR_NULL_POINTER;
  if (any_off({x, planes}, 15)) return QUIP_ERR_MISALIGNED;
  return x_to_planes_linear_launch(x, planes, k, (hipStream_t)stream);
}

// (the one GEMV entry that answers the alignment -- the table's 64 bytes too -- before gemv_launch looks at k, and n == 0
//  behind the NULL check, where quip_e8p_gemv_planes_ws answers n == 0 before everything: ABI as recorded)
int quip_e8p_gemv_planes(const void* planes, const void* qidxs, const void* grid, void* y, int32_t n,
                         int32_t k, quip_stream_t stream) {
  if (any_null({planes, qidxs, grid, y})) return QUIP_ERR_NULL_POINTER;
  if (n < 0) return QUIP_ERR_BAD_SHAPE;
  if (n == 0) return QUIP_OK;
  if (any_off({planes, qidxs}, 15) || any_off({grid}, kGemvE8P.grid_mask)) return QUIP_ERR_MISALIGNED;
  return gemv_launch(kGemvE8P, &planes, &qidxs, grid, nullptr, &y, &n, 1, k, nullptr, 0, stream);
}

int quip_e8p_mm_skinny(const void* x, const void* qidxs, const void* grid, void* y, int32_t m, int32_t n, int32_t k,
                       quip_stream_t stream) {
  return mm_skinny(kE8P, x, qidxs, {grid}, y, m, n, k, stream);
}

int quip_e8prvq4_mm_skinny(const void* x, const void* qidxs, const void* grid, float resid_scale, void* y, int32_t m,
                           int32_t n, int32_t k, quip_stream_t stream) {
  return mm_skinny(kE8PRVQ4, x, qidxs, {grid, nullptr, resid_scale}, y, m, n, k, stream);
}

int quip_e8prvq3_mm_skinny(const void* x, const void* qidxs, const void* grid, const void* e81b_packed, float resid_scale,
                           void* y, int32_t m, int32_t n, int32_t k, quip_stream_t stream) {
  return mm_skinny(kE8PRVQ3, x, qidxs, {grid, e81b_packed, resid_scale}, y, m, n, k, stream);
}

int quip_d4_mm_skinny(const void* x, const void* qidxs, const void* grid_f16, void* y, int32_t m, int32_t n, int32_t k,
                      quip_stream_t stream) {
  return mm_skinny(kD4, x, qidxs, {grid_f16}, y, m, n, k, stream);
}

int quip_hi_mm_skinny(const void* x, const void* qidxs, void* y, int32_t m, int32_t n, int32_t k, quip_stream_t stream) {
  return mm_skinny(kHI, x, qidxs, {}, y, m, n, k, stream);
}

int quip_e8p_mm_batched(const void* x, const void* qidxs, const void* grid, void* y, int64_t m, int32_t n, int32_t k,
                        quip_stream_t stream) {
  return mm_batched(kE8P, x, qidxs, {grid}, y, m, n, k, stream);
}

int quip_e8prvq4_mm_batched(const void* x, const void* qidxs, const void* grid, float resid_scale, void* y, int64_t m,
                            int32_t n, int32_t k, quip_stream_t stream) {
  return mm_batched(kE8PRVQ4, x, qidxs, {grid, nullptr, resid_scale}, y, m, n, k, stream);
}

int quip_e8prvq3_mm_batched(const void* x, const void* qidxs, const void* grid, const void* e81b_packed, float resid_scale,
                            void* y, int64_t m, int32_t n, int32_t k, quip_stream_t stream) {
  return mm_batched(kE8PRVQ3, x, qidxs, {grid, e81b_packed, resid_scale}, y, m, n, k, stream);
}

int quip_d4_mm_batched(const void* x, const void* qidxs, const void* grid_f16, void* y, int64_t m, int32_t n, int32_t k,
                       quip_stream_t stream) {
  return mm_batched(kD4, x, qidxs, {grid_f16}, y, m, n, k, stream);
}

int quip_hi_mm_batched(const void* x, const void* qidxs, void* y, int64_t m, int32_t n, int32_t k, quip_stream_t stream) {
  return mm_batched(kHI, x, qidxs, {}, y, m, n, k, stream);
}

int quip_e8p_mm_origorder_ws(const void* x, const void* qidxs, const void* grid, void* y, int32_t m,
                             int32_t n, int32_t k, void* workspace, size_t workspace_bytes,
                             quip_stream_t stream) {
  if (!any_null({x, qidxs, grid, y, workspace}) && m >= 1 && m < 32 && n > 0 && e8p_gemv_mfma_supported(n, k) &&
      !any_off({x, qidxs, workspace}, 15) && aligned64(grid) && workspace_bytes >= (size_t)m * e8p_gemv_mfma_planes_bytes(k)) {
    // 1 <= M < 32 on the matrix cores: digit planes of every row, then passes of up to
    // e8p_gemv_mfma_max_rows rows over the codes (M == 1: the plain GEMV)
    const int rc = x_to_planes_linear_launch(x, workspace, k, (hipStream_t)stream, m);
    if (rc != QUIP_OK) return rc;
    if (m == 1) return e8p_gemv_mfma_launch(workspace, qidxs, grid, y, n, k, GemvTune{}, (hipStream_t)stream);
    const int per = e8p_gemv_mfma_max_rows(n, k);
    const size_t pstride = e8p_gemv_mfma_planes_bytes(k);
    for (int r0 = 0; r0 < m; r0 += per) {
      const int mr = m - r0 < per ? m - r0 : per;
      const int rc2 = e8p_gemv_mfma_rows_launch(reinterpret_cast<const char*>(workspace) + (size_t)r0 * pstride, qidxs,
                                                grid, reinterpret_cast<char*>(y) + (size_t)r0 * n * 2, mr, n, k,
                                                GemvTune{}, (hipStream_t)stream);
      if (rc2 != QUIP_OK) return rc2;
    }
    return QUIP_OK;
  }
  return quip_e8p_mm_origorder(x, qidxs, grid, y, m, n, k, stream);
}

int quip_e8p_x_to_planes_laneorder(const void* x, void* planes, int32_t k, quip_stream_t stream) {
  if (!x || !planes) return QUIP_ERR_NULL_POINTER;
  return x_to_planes_launch(x, planes, k, (hipStream_t)stream);
}

// ---- the tuning hooks (micro-benchmarks only, not in the public header) ------------------------------------------------
int quip_e8p_gemv_tuned(const void* x, const void* qidxs, const void* grid, void* y, int32_t n,
                        int32_t k, int32_t kernel, int32_t rep, int32_t rows, int32_t blocks,
                        int32_t waves_g, int32_t max_waves, int32_t digits, void* dbg,
                        quip_stream_t stream) {
  if (any_null({x, qidxs, grid, y})) return QUIP_ERR_NULL_POINTER;
  const GemvTune t = tune_of(rep, rows, blocks, waves_g, max_waves, digits, dbg);
  if (kernel == 2) return stream_probe_launch(qidxs, y, n, k, t, (hipStream_t)stream);
  if (kernel == 5) return pattern_probe_launch(qidxs, y, n, k, t, (hipStream_t)stream);
  if (kernel == 6) return shape_probe_launch(qidxs, y, n, k, t, (hipStream_t)stream);
  if (kernel == 4) return e8p_gemv_mfma_launch(x, qidxs, grid, y, n, k, t, (hipStream_t)stream);
  // kernel 4: matrix-core GEMV on linear digit planes; kernel 0: VALU integer GEMV on lane-ordered
  // digit planes; kernel 3: the same converting fp16 x itself
  return e8p_gemv_i8_launch(x, kernel == 3 ? 1 : 0, qidxs, grid, y, n, k, t, (hipStream_t)stream);
}

int quip_e8p_gemv_v2_tuned(const void* planes, const void* qidxs, const void* grid, void* y, void* ws, int32_t n,
                           int32_t k, int32_t rep2, int32_t slots, int32_t blocks, int32_t ksplit,
                           int32_t max_waves, int32_t runlen, void* dbg, quip_stream_t stream) {
  if (any_null({planes, qidxs, grid, y})) return QUIP_ERR_NULL_POINTER;
  return gemv_v2_auto(&planes, &qidxs, grid, &y, ws, &n, 1, k, tune_of(rep2, slots, blocks, ksplit, max_waves, runlen, dbg),
                      (hipStream_t)stream);
}

int quip_e8p_gemv_v2_group_tuned(const void* const* planes, const void* const* qidxs, const void* grid,
                                 void* const* ys, void* ws, const int32_t* ns, int32_t count, int32_t k, int32_t rep,
                                 int32_t slots, int32_t blocks, int32_t ksplit, int32_t max_waves, int32_t runlen,
                                 void* dbg, quip_stream_t stream) {
  if (any_null({planes, qidxs, grid, ys, ns})) return QUIP_ERR_NULL_POINTER;
  if (count < 1 || count > QUIP_MAX_GROUP) return QUIP_ERR_UNSUPPORTED;
  return gemv_v2_auto(planes, qidxs, grid, ys, ws, ns, count, k, tune_of(rep, slots, blocks, ksplit, max_waves, runlen, dbg),
                      (hipStream_t)stream);
}

size_t quip_e8p_gemv_v2_workspace_bytes(int32_t n) { return e8p_gemv_v2_workspace_words(n) * 4; }

int quip_e8p_gemv_fused_tuned(const quip_gemv_fused_in* in, const void* const* qidxs, const void* grid,
                              void* const* ys, const int32_t* ns, int32_t count, int32_t k, void* dbg,
                              quip_stream_t stream) {
  return e8p_gemv_mfma_fused_launch(fused_in_of(in, count), qidxs, grid, ys, ns, count, k, tune_of(0, 0, 0, 0, 0, 0, dbg),
                                    (hipStream_t)stream);
}

int quip_e8p_gemv_group_tuned(const void* const* planes, const void* const* qidxs, const void* grid,
                              void* const* ys, const int32_t* ns, int32_t count, int32_t k, int32_t rep,
                              int32_t rows, int32_t blocks, int32_t max_waves, void* dbg,
                              quip_stream_t stream) {
  return e8p_gemv_mfma_group_launch(planes, qidxs, grid, ys, ns, count, k, tune_of(rep, rows, blocks, 0, max_waves, 0, dbg),
                                    (hipStream_t)stream);
}

int quip_e8prvq3_mm_origorder(const void* x, const void* qidxs, const void* grid,
                              const void* grid2, float scale, void* y, int32_t m, int32_t n,
                              int32_t k, quip_stream_t stream) {
  return mm_origorder(kE8PRVQ3, x, qidxs, {grid, grid2, scale}, y, m, n, k, stream);
}

int quip_e8prvq4_mm_origorder(const void* x, const void* qidxs, const void* grid, float scale,
                              void* y, int32_t m, int32_t n, int32_t k, quip_stream_t stream) {
  return mm_origorder(kE8PRVQ4, x, qidxs, {grid, nullptr, scale}, y, m, n, k, stream);
}

int quip_d4_mm_origorder(const void* x, const void* qidxs, const void* grid_f16, void* y,
                         int32_t m, int32_t n, int32_t k, quip_stream_t stream) {
  return mm_origorder(kD4, x, qidxs, {grid_f16}, y, m, n, k, stream);
}

int quip_hi_mm_origorder(const void* x, const void* qidxs, void* y, int32_t m, int32_t n,
                         int32_t k, quip_stream_t stream) {
  return mm_origorder(kHI, x, qidxs, {}, y, m, n, k, stream);
}

int quip_decompress_e8p_origorder(const void* qidxs, const void* grid, void* w, int64_t rows,
                                  int32_t k, quip_stream_t stream) {
  return decompress_origorder(kE8P, qidxs, {grid}, w, rows, k, stream);
}

int quip_decompress_e8prvq3_origorder(const void* qidxs, const void* grid, const void* grid2,
                                      float scale, void* w, int64_t rows, int32_t k,
                                      quip_stream_t stream) {
  return decompress_origorder(kE8PRVQ3, qidxs, {grid, grid2, scale}, w, rows, k, stream);
}

int quip_decompress_e8prvq4_origorder(const void* qidxs, const void* grid, float scale, void* w,
                                      int64_t rows, int32_t k, quip_stream_t stream) {
  return decompress_origorder(kE8PRVQ4, qidxs, {grid, nullptr, scale}, w, rows, k, stream);
}

int quip_decompress_d4_origorder(const void* qidxs, const void* grid_f16, void* w, int64_t rows,
                                 int32_t k, quip_stream_t stream) {
  return decompress_origorder(kD4, qidxs, {grid_f16}, w, rows, k, stream);
}

int quip_decompress_hi_origorder(const void* qidxs, void* w, int64_t rows, int32_t k,
                                 quip_stream_t stream) {
  return decompress_origorder(kHI, qidxs, {}, w, rows, k, stream);
}

}  // extern "C"
