// Internal (non-ABI) declarations shared by the translation units of libquip_mi355.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/quip_mi355.h"

namespace quip {

int device_cu_count();
// Persistent launches (decode_engine.hip, decode_block*.hip) spin across workgroups: every one of the `nwg` workgroups has to be
// resident at once.  True when the current device has at least nwg CUs (no fall-back value: a failed query says no) and the
// occupancy query admits the grid for this kernel / block size / dynamic LDS.  Cached per kernel and device (launch.hip.h).
struct ResidencyCache { signed char ok[16] = {}; };      // 0 unknown, 1 fits, -1 does not
bool persistent_grid_fits(ResidencyCache& cache, const void* kernel, int threads, int lds, int nwg);
int device_cu_count_strict();                            // 0 when the query fails

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: the one DynLdsCache per kernel
// instantiation (launch.hip.h) remembers the largest size configured on each device of the process, so a
// process that drives several GPUs configures the kernel on each of them.  (Benign race: the attribute is idempotent.)
struct DynLdsCache { int bytes[16] = {}; };
int ensure_dyn_lds(DynLdsCache& cache, const void* kernel, int lds);   // QUIP_OK / QUIP_ERR_LAUNCH

// Environment switches are integers, read once per process: static const int v = env_int("QUIP_X", dflt) at the point of use.
int env_int(const char* name, int dflt);
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Tuning knobs of the E8P decode GEMV (0 = pick automatically).  Exposed through
// quip_e8p_gemv_tuned() for the micro-benchmark only; the ABI entry points use auto.
struct GemvTune {
  int rep = 0;        // LDS table replication: 1 or 32 (i8 kernel) / 1 or 16 (f16 kernel)
  int rows = 0;       // rows in flight per wave iteration: 1, 2 or 4
  int blocks = 0;     // workgroups
  int waves_g = 0;    // row-groups per workgroup (waves = waves_g * J)
  int max_waves = 0;  // cap on waves per workgroup (default 16)
  int digits = 0;     // i8 kernel: int8 digit planes of x, 2 or 3 (default 3)
  const void* grid2 = nullptr;   // matrix-core GEMV, rep == 40 (E8P12RVQ3B): the E81B table, 256 x 8 int8 (4r)
  void* dbg = nullptr;  // i8 kernel: device buffer of 8 x uint64 s_memtime stamps per workgroup
};
int stream_probe_launch(const void* qidxs, void* out, int n, int k, const GemvTune& tune,
                        hipStream_t stream);

bool e8p_gemv_i8_supported(int n, int k);
size_t e8p_gemv_planes_bytes(int k);
int x_to_planes_launch(const void* x, void* planes, int k, hipStream_t stream);
// xmode 0: xsrc = digit planes (+ shift word), xmode 1: xsrc = fp16 x (self-contained, slower)
int e8p_gemv_i8_launch(const void* xsrc, int xmode, const void* qidxs, const void* grid, void* y,
                       int n, int k, const GemvTune& tune, hipStream_t stream);
// matrix-core GEMV (default bs=1 path): planes = [3][Kp] digit bytes + shift word
bool e8p_gemv_mfma_supported(int n, int k);
size_t e8p_gemv_mfma_planes_bytes(int k);
int x_to_planes_linear_launch(const void* x, void* planes, int k, hipStream_t stream, int rows = 1);
int e8p_gemv_mfma_launch(const void* planes, const void* qidxs, const void* grid, void* y, int n, int k,
                         const GemvTune& tune, hipStream_t stream);
// second-generation matrix-core GEMV (e8p_gemv_v2.hip): whole-line loads, K split over workgroups.
// ws: zeroed int32 workspace of e8p_gemv_v2_workspace_words(n) words (needed when K is split; left zeroed).
// tune: rep = 32 / 24 / 16 -> (32, 32) / (32, 16) / (16, 16) table copies, rows = load slots per wave,
// waves_g = K split, digits = segments per run, blocks, max_waves (0: automatic); rep = 4: nibble mode (below)
bool e8p_gemv_v2_supported(int n, int k);
size_t e8p_gemv_v2_workspace_words(int n);
int e8p_gemv_v2_group_launch(const void* const* planes, const void* const* qidxs, const void* grid, void* const* ys,
                             void* ws, const int* ns, int count, int k, const GemvTune& tune, hipStream_t stream);
// the same kernel in nibble mode (e8p_gemv_v2n.hip; tune.rep == 4): 4-byte table entries, 64 KB of tables whatever K is
int e8p_gemv_v2n_group_launch(const void* const* planes, const void* const* qidxs, const void* grid, void* const* ys,
                              void* ws, const int* ns, int count, int k, const GemvTune& tune, hipStream_t stream);
int shape_probe_launch(const void* qidxs, void* out, int n, int k, const GemvTune& tune, hipStream_t stream);
int pattern_probe_launch(const void* qidxs, void* out, int n, int k, const GemvTune& tune, hipStream_t stream);

// The one numbering of the codebooks below the ABI: every product launcher switches on it.  Two kernel-facing numberings
// stay beside it, each mapped at one place: GemvTune::rep (the GEMV kernels' table mode 0 / 64 / 40: the GemvMode constants
// of capi.hip) and BlockEngineArgs::codebook (0..5, the public quip_block_engine_args::codebook handed through).
enum CodebookId { kE8P = 0, kE8PRVQ3 = 1, kE8PRVQ4 = 2, kD4 = 3, kHI = 4 };

struct CodebookArgs {
  const void* grid = nullptr;   // grid_packed_abs (E8P*), fp16 grid (D4)
  const void* grid2 = nullptr;  // e81b_grid_packed (RVQ3)
  float scale = 0.f;            // residual scale (RVQ3/4)
};

int generic_mm_launch(CodebookId cb, const void* x, const void* qidxs, const CodebookArgs& a,
                      void* y, int m, int n, int k, hipStream_t stream);
int decompress_launch(CodebookId cb, const void* qidxs, const CodebookArgs& a, void* w,
                      int64_t rows, int k, hipStream_t stream);
// The Hadamard transform launches (hadamard.hip): `count` problems -- the public quip_had_problem is the record inside the
// library too -- of one n, K, transpose and kind (planes / fp16 rows) in one launch.  Every C entry point ends here.
int had_transform_group_launch(const quip_had_problem* problems, int count, bool planes, int64_t rows, int n, int K,
                               int transpose, hipStream_t stream);
// the same validation, then the plan of the launch (of its first 65535 rows) for a device of `cus` CUs instead of the
// launch; out[kHadPlanInts] as quip_had_plan() documents it
constexpr int kHadPlanInts = 7 + 6 * QUIP_MAX_GROUP;
int had_transform_group_plan(const quip_had_problem* problems, int count, bool planes, int64_t rows, int n, int K,
                             int transpose, int cus, int32_t* out);
const char* had_plan_kind_name(int kind);   // the instantiation as text, null past the last kind
// quantise-time nearest E8P12 codeword (quantize.hip): x fp32 (nvec, 8) -> vals fp32 (nvec, 8), idx int64 (nvec)
int e8p_quantize_launch(const void* x, int64_t nvec, const void* grid_packed_abs, void* vals, void* idx,
                        hipStream_t stream);
// one LDLQ panel of c <= 128 columns (quantize.hip): A, B fp32 (m, c), M fp32 (c, c), P fp32 (c / 8, 8, 8) or null ->
// hat fp32 (m, c), idx int64 (m, c / 8)
int ldlq_panel_launch(const void* A, const void* B, const void* M, const void* P, int64_t m, int c,
                      const void* grid_packed_abs, void* hat, void* idx, hipStream_t stream);
// the same with the two-stage step of the residual codebooks: resid_grid null = E8P12RVQ4B (idx = a << 16 | b), fp32 (256, 8)
// = E8P12RVQ3B (idx = a << 8 | b); hat = a + b * resid_scale
int ldlq_panel_rvq_launch(const void* A, const void* B, const void* M, const void* P, int64_t m, int c,
                          const void* grid_packed_abs, const void* resid_grid, float resid_scale, void* hat, void* idx,
                          hipStream_t stream);
// rows mode: up to e8p_gemv_mfma_max_rows(n, k) <= 5 activation rows against one matrix in one pass
int e8p_gemv_mfma_max_rows(int n, int k, int mode = 0);   // mode: 0 E8P12, 64 D4 / HI, 40 E8P12RVQ3B (2k virtual)
int e8p_gemv_mfma_rows_launch(const void* planes, const void* qidxs, const void* grid, void* y, int mrows, int n,
                              int k, const GemvTune& tune, hipStream_t stream);
bool e8p_gemv_mfma_group_supported(const int* ns, int count, int k);
int e8p_gemv_mfma_group_launch(const void* const* planes, const void* const* qidxs, const void* grid,
                               void* const* ys, const int* ns, int count, int k, const GemvTune& tune,
                               hipStream_t stream);
// input side of a bs=1 GEMV computed in its prologue (see FusedIn in e8p_gemv_mfma.hip)
struct GemvFusedIn {
  const void* x = nullptr;         // fp16 [k]: the activation (when z == null)
  const void* z = nullptr;         // fp16 [k]: producer's GEMV output, still to be output-transformed
  const void* post = nullptr;      // fp16 [k]: producer's SV            (z != null)
  const void* residual = nullptr;  // fp16 [k] or null: added to the producer's output
  void* h_out = nullptr;           // fp16 [k]: receives the producer's output (z != null)
  const void* rms_w = nullptr;     // fp16 [k] or null: RMSNorm weight
  const void* pre[3] = {nullptr, nullptr, nullptr};   // SU of every problem
  float scale[3] = {1.f, 1.f, 1.f};                   // wscale / sqrt(k)
  float z_scale = 1.f, rms_eps = 1e-5f;
};
bool e8p_gemv_mfma_fused_supported(const int* ns, int count, int k);
int e8p_gemv_mfma_fused_launch(const GemvFusedIn& in, const void* const* qidxs, const void* grid,
                               void* const* ys, const int* ns, int count, int k, const GemvTune& tune,
                               hipStream_t stream);
// fused dequant + MFMA GEMM for batches (e8p_prefill_gemm.hip): y (m, n) = x (m, k) @ decode(qidxs)^T.  The codes per
// codebook: E8P12 int16 (n, k / 8); E8P12RVQ4B int32 (main << 16 | residual), weight = fma(a.scale, w_resid, w_main) in fp16;
// E8P12RVQ3B 3-byte codes (n, 3 k / 8 bytes), a.grid2 = the packed E81B table, uint32 [256] (eight int4 = 2 x value per
// entry); D4 one-byte codes (n, k / 4), a.grid = the fp16 (256, 4) table; HI int32 codes of eight nibbles, no table
bool e8p_prefill_gemm_supported(int64_t m, int n, int k);
int prefill_gemm_launch(CodebookId cb, const void* x, const void* qidxs, const CodebookArgs& a, void* y, int64_t m, int n,
                        int k, hipStream_t stream);
// single-pass skinny product, 1 <= m <= 32 * 65535 rows, fp16 MFMA (e8p_skinny_gemm.hip): the same codes and tables
bool e8p_skinny_gemm_supported(int m, int n, int k);
int skinny_gemm_launch(CodebookId cb, const void* x, const void* qidxs, const CodebookArgs& a, void* y, int m, int n, int k,
                       hipStream_t stream);
// bf16 / fp32 (and plain fp16) Walsh-Hadamard transform of the last dimension (hadamard_generic.hip)
int hadamard_generic_launch(const void* x, void* y, int64_t rows, int n, float scale, int dtype, hipStream_t stream);
// The attention launches (decode_glue.hip and the headers it includes).  They share their operands: q, k (before the
// rotation) and v of the new token(s), the rotary tables (max_len, head_dim), the position(s) on the device, the cache
// (or, paged, the two pools) and out -- AttnIO -- and their sizes -- AttnShape; what a variant adds comes beside them.
// Every launcher answers BAD_SHAPE before UNSUPPORTED; pointers are the C entry points' business (capi.hip).
struct AttnIO {
  const void *q, *k, *v;
  const float *cos, *sin;
  const int64_t* pos;
  void *kcache, *vcache, *out;
};
struct AttnShape {
  int batch;                   // sequences (cache slots); 1: the bs = 1 launches and the chunk launch
  int heads, kv_heads, head_dim, max_len;
  int window;                  // sliding window, 0: none
  float scale;
};
// a paged cache: kcache / vcache of AttnIO are pools (n_pages, kv_heads, 64, head_dim), table (batch, max_pages) int32 on the
// device.  The _f8 launches: pools of e4m3fn bytes, a byte c means e4m3fn(c) * 2^k_exp / 2^v_exp, exponents in [-8, 7];
// the launches on fp16 pools take 0, 0
struct AttnPages {
  const int32_t* table;
  int n_pages, max_pages;
  int k_exp, v_exp;
};
// the segments of a ragged launch (host arrays): segment s is seg_rows[s] rows that continue slot seg_slot[s]
struct AttnSegments {
  const int32_t *slot, *rows;
  int nseg;
};
// per-head RMSNorm of q and of the new k row in front of the rotation (qk_norm.hip.h)
struct AttnQkNorm {
  const void *qw, *kw;
  float eps;
};
size_t rope_attn_workspace_bytes(int heads, int head_dim);
size_t rope_attn_batched_workspace_bytes(int batch, int heads, int head_dim);
// bs = 1: one token against the cache (kv_heads, max_len, head_dim)
int rope_attn_decode_launch(const AttnIO& io, const AttnShape& s, hipStream_t stream, void* workspace);
int rope_attn_decode_qknorm_launch(const AttnIO& io, const AttnShape& s, const AttnQkNorm& norm, hipStream_t stream,
                                   void* workspace);
// the same from the raw GEMV outputs z[3] of q / k / v_proj and their SV vectors post[3] (io.q / k / v unused)
bool rope_attn_decode_z_supported(int heads, int kv_heads, int head_dim);
int rope_attn_decode_z_launch(const void* const* z, const void* const* post, const float* scales, const AttnIO& io,
                              const AttnShape& s, hipStream_t stream, void* workspace);
// batched decode: s.batch sequences, each at its own position, in one launch; start: sequences that begin at cache row
// start[b] (left-padded batches), row t has rotary position t - start[b]
int rope_attn_decode_batched_launch(const AttnIO& io, const AttnShape& s, hipStream_t stream, void* workspace);
int rope_attn_decode_batched_start_launch(const AttnIO& io, const int64_t* start, const AttnShape& s, hipStream_t stream,
                                          void* workspace);
int rope_attn_decode_batched_qknorm_launch(const AttnIO& io, const AttnShape& s, const AttnQkNorm& norm, hipStream_t stream,
                                           void* workspace);
int rope_attn_decode_paged_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, hipStream_t stream,
                                  void* workspace);
int rope_attn_decode_paged_f8_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, hipStream_t stream,
                                     void* workspace);
// chunk_attn.hip.h: rows queries at positions [*pos, *pos + rows) against cache rows [0, *pos + rows); ragged_attn.hip.h /
// paged_attn.hip.h: the same for segments of the rows, each continuing one slot of a batched (paged) cache at pos[slot]
int rope_attn_chunk_launch(const AttnIO& io, const AttnShape& s, int rows, hipStream_t stream);
int rope_attn_ragged_launch(const AttnIO& io, const AttnShape& s, int rows, const AttnSegments& segs, hipStream_t stream);
int rope_attn_ragged_paged_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, int rows,
                                  const AttnSegments& segs, hipStream_t stream);
int rope_attn_ragged_paged_f8_launch(const AttnIO& io, const AttnPages& pages, const AttnShape& s, int rows,
                                     const AttnSegments& segs, hipStream_t stream);
// qk_norm.hip.h: per-head RMSNorm of q (rows, heads * head_dim) and k (rows, kv_heads * head_dim) in place
int qk_norm_rows_launch(void* q, void* k, const void* qw, const void* kw, int64_t rows, int heads, int kv_heads,
                        int head_dim, float eps, hipStream_t stream);
// the greedy tail (decode_glue.hip): tok <- arg-max of the logits (of every row), pos += 1
int argmax_step_launch(const void* logits, int n, void* tok, void* pos, hipStream_t stream);
int argmax_step_batched_launch(const void* logits, int batch, int n, void* tok, void* pos, hipStream_t stream);
// nll_rows.hip.h (in decode_glue.hip): per row of (rows, n) fp16 logits the log-sum-exp, the log-probability of target[row] and
// the arg-max; lse / argmax may be null
int nll_rows_launch(const void* logits, int rows, int n, const int64_t* target, float* logprob, float* lse,
                    int64_t* argmax, hipStream_t stream);
// sample_rows.hip.h (in decode_glue.hip): per row of (rows, n) fp16 logits one token by the row's own temperature, top-k,
// top-p and seed at counter pos[row]; tok[row] = token, pos[row] += 1; kept may be null
int sample_rows_launch(const void* logits, int rows, int n, const float* temperature, const int32_t* top_k,
                       const float* top_p, const int64_t* seed, int64_t* tok, int64_t* pos, int32_t* kept,
                       hipStream_t stream);
// spec_rows.hip.h (in decode_glue.hip): the step of a speculative greedy decode between two chunk passes of k + 1 rows, one
// workgroup.  _draft: the guesses behind rows_tok[0] at pos (the first pass of a call); _accept_draft: accept the guesses
// that nll_rows' arg-max confirmed, emit, rewind pos, then the same draft.  pred may be null where pred_cap is 0
int spec_draft_launch(int64_t* rows_tok, int32_t* n_draft, int64_t* pos, int64_t* hist, int hist_cap, const int64_t* pred,
                      const int32_t* n_pred, int pred_cap, int64_t* stats, int k, int gmin, int gmax, hipStream_t stream);
int spec_accept_draft_launch(const int64_t* argmax, const float* lse, int64_t* rows_tok, int32_t* n_draft, int64_t* pos,
                             int64_t* hist, int hist_cap, const int64_t* pred, const int32_t* n_pred, int pred_cap,
                             int64_t* out, int64_t* out_len, int cap_out, int64_t* stats, int k, int gmin, int gmax,
                             hipStream_t stream);
// lora_rows.hip.h (in decode_glue.hip): t = A[row_adapter[row]] xin(row) over (rows, in) fp16 rows (mode 0 x, 1 RMSNorm(x) w with
// aux = w, 2 x silu(aux row)), and y_j += scale B_j t for up to three segments; rows without an adapter: zeros / untouched
int lora_shrink_rows_launch(const void* x, const void* A, const int32_t* row_adapter, float* t, int64_t rows, int in, int R,
                            int n_adapters, int mode, const void* aux, float eps, hipStream_t stream);
int lora_expand_rows_launch(const float* t, const int32_t* row_adapter, const float* scale, int64_t rows, int Rt, int n_adapters,
                            int segments, void* const* y, const void* const* B, const int32_t* out, const int32_t* R,
                            const int32_t* r0, hipStream_t stream);
// persistent decode engine, stage 1 (decode_engine.hip): GEMV[gate, up] -> output transforms -> SiLU product ->
// input transform of down -> GEMV[down] of one decoder block in one launch
struct FfnEngineArgs {
  const void* w_gate = nullptr;      // Qidxs (n_ffn, hidden / 8) int16
  const void* w_up = nullptr;
  const void* w_down = nullptr;      // Qidxs (hidden, n_ffn / 8) int16
  const void* planes_gate = nullptr; // digit planes of gate's / up's transformed input (3 Kp + 16 bytes each)
  const void* planes_up = nullptr;
  const void* had3 = nullptr;        // fp16: gate.had_right, up.had_right (K x K row major, each padded to a multiple of 8 elements), down.had_left transposed, zero padded to (K16, K16), K16 = K rounded up to 16
  const void* sv_gate = nullptr;     // fp16 [n_ffn]
  const void* sv_up = nullptr;
  const void* su_down = nullptr;     // fp16 [n_ffn]
  void* z_down = nullptr;            // fp16 [hidden]: raw product of down_proj
  const void* grid = nullptr;        // grid_packed_abs
  void* workspace = nullptr;         // ffn_engine_workspace_bytes(), zeroed once at allocation
  void* dbg = nullptr;               // optional: 16 uint64 s_memtime stamps per workgroup
  float out_scale = 1.f;             // 1 / sqrt(L), L = n_ffn / K
  float in_scale = 1.f;              // down.wscale_float / sqrt(L)
  int hidden = 0, n_ffn = 0, K = 0;
};
bool ffn_engine_supported(int hidden, int n_ffn, int K);
size_t ffn_engine_workspace_bytes(int n_ffn, int K);
int ffn_engine_launch(const FfnEngineArgs& in, hipStream_t stream);
// persistent decode engine, stage 2 (decode_block.hip): consecutive decoder blocks of a Llama-2-7B-shaped model, one token
struct BlockEngineArgs {
  const void* layers = nullptr;      // n_layers descriptors of block_engine_layer_bytes() bytes each (device memory)
  const void* h_in = nullptr;        // fp16 [hidden]
  void* h_out = nullptr;             // fp16 [hidden]
  const void* pos = nullptr;         // int64 device scalar
  const float* cos = nullptr;        // fp32 [max_len, head_dim]
  const float* sin = nullptr;
  const void* grid = nullptr;        // grid_packed_abs
  void* workspace = nullptr;         // block_engine_workspace_bytes(), zeroed once
  void* dbg = nullptr;
  int n_layers = 0, max_len = 0, dbg_layer = -1;
  float rms_eps = 1e-5f, attn_scale = 1.f;
  int codebook = 0;                  // 0: E8P12 (grid = grid_packed_abs), 1: D4 (grid = the fp16 (256, 4) table), 2: E8P12RVQ4B, 3: HI (grid = the byte table), 4: E8P12RVQ3B, 5: E8P12 on launch-tiled codes (shape 0)
  float resid_scale = 0.f;           // codebooks 2, 4: the fp16 residual scale
  const void* grid2 = nullptr;       // codebook 4 (E8P12RVQ3B): int8 (256, 8) E81B table
  // the whole token in the launch (token_tail.hip.h; shapes 0 and 2).  lm_head == nullptr: blocks only, h_in -> h_out.  Else
  // h_in is row *tok of embed, and the launch writes logits, the arg-max into *tok and *pos + 1 into *pos (h_out may be null)
  void* tok = nullptr;               // int64 device scalar
  const void* embed = nullptr;       // fp16 [vocab, hidden]
  const void* final_norm = nullptr;  // fp16 [hidden]
  const void* lm_head = nullptr;     // fp16 [vocab, hidden]
  void* logits = nullptr;            // fp16 [vocab]
  void* xnorm = nullptr;             // optional: fp16 [hidden], the normalised hidden state (debug)
  int vocab = 0;
};
bool block_engine_supported(int hidden, int heads, int kv_heads, int head_dim, int n_ffn, int K);
size_t block_engine_workspace_bytes();
size_t block_engine_layer_bytes();
int block_engine_launch(const BlockEngineArgs& in, hipStream_t stream);
// shape 0, codebook 5: E8P12 with the code matrices in the launch-tiled layout (decode_block.hip compiled with QUIP_BLOCK_TILED:
// decode_block_tiled.hip); block_engine_launch hands it over
int block_engine_tiled_launch(const BlockEngineArgs& in, hipStream_t stream);
// the same for the grouped-query 8192-wide shape (decode_block_gqa.hip: Llama-2-70B; E8P12): its own descriptor vectors
// (permuted, see include/quip_mi355.h) and workspace
bool block_engine_gqa_supported(int hidden, int heads, int kv_heads, int head_dim, int n_ffn, int K);
size_t block_engine_gqa_workspace_bytes();
size_t block_engine_gqa_layer_bytes();
int block_engine_gqa_launch(const BlockEngineArgs& in, hipStream_t stream);
// the 4096-wide grouped-query shape (Llama-3-8B / Mistral-7B): decode_block.hip compiled with QUIP_BLOCK_G8 (decode_block_g8.hip)
bool block_engine_g8_supported(int hidden, int heads, int kv_heads, int head_dim, int n_ffn, int K);
size_t block_engine_g8_workspace_bytes();
int block_engine_g8_launch(const BlockEngineArgs& in, hipStream_t stream);

}  // namespace quip

// kernel: 4 = matrix-core GEMV (default), 0 / 3 = VALU integer GEMV (planes / fp16 x), 2 / 5 = read probes
extern "C" int quip_e8p_gemv_tuned(const void* x, const void* qidxs, const void* grid, void* y,
                                   int32_t n, int32_t k, int32_t kernel, int32_t rep, int32_t rows,
                                   int32_t blocks, int32_t waves_g, int32_t max_waves,
                                   int32_t digits, void* dbg, quip_stream_t stream);
extern "C" int quip_e8p_gemv_fused_tuned(const quip_gemv_fused_in* in, const void* const* qidxs, const void* grid,
                                         void* const* ys, const int32_t* ns, int32_t count, int32_t k,
                                         void* dbg, quip_stream_t stream);
extern "C" int quip_e8p_gemv_group_tuned(const void* const* planes, const void* const* qidxs, const void* grid,
                                         void* const* ys, const int32_t* ns, int32_t count, int32_t k,
                                         int32_t rep, int32_t rows, int32_t blocks, int32_t max_waves,
                                         void* dbg, quip_stream_t stream);
extern "C" int quip_e8p_gemv_v2_tuned(const void* planes, const void* qidxs, const void* grid, void* y, void* ws,
                                      int32_t n, int32_t k, int32_t rep2, int32_t slots, int32_t blocks,
                                      int32_t ksplit, int32_t max_waves, int32_t runlen, void* dbg, quip_stream_t stream);
extern "C" int quip_e8p_gemv_v2_group_tuned(const void* const* planes, const void* const* qidxs, const void* grid,
                                            void* const* ys, void* ws, const int32_t* ns, int32_t count, int32_t k,
                                            int32_t rep, int32_t slots, int32_t blocks, int32_t ksplit,
                                            int32_t max_waves, int32_t runlen, void* dbg, quip_stream_t stream);
extern "C" size_t quip_e8p_gemv_v2_workspace_bytes(int32_t n);
// the plan e8p_gemv_v2_group_launch makes for these tuning arguments (rep 4: nibble mode), without a launch: out[13] = rc, rep, slots,
// ksplit, nrb, spw, rpb[3], runlen, rpr_inv, threads, lds (e8p_gemv_v2_plan.hip.h); have_grid2 / have_ws: the E81B table /
// a workspace would be passed.  Pure host arithmetic: the same answer with and without a GPU of 256 CUs
extern "C" int quip_e8p_gemv_v2_plan(const int32_t* ns, int32_t count, int32_t k, int32_t rep, int32_t slots,
                                     int32_t blocks, int32_t ksplit, int32_t max_waves, int32_t runlen,
                                     int32_t have_grid2, int32_t have_ws, int32_t* out);
// the plan quip_had_transform_group_f16 (planes == 0) / quip_had_transform_planes_group and _planes_rows (planes != 0) make
// for these arguments, without a launch; pointers are looked at (NULL, alignment), never dereferenced.  Returns what the
// entry point would, up to the launch.  out[25] = rc, kind, grid x / y / z, threads, lds, then per problem pp, tgroups,
// part_off, chain_off, vec, vec_out; kind -1 and zeros when nothing would be launched.  quip_had_plan_kind_name(kind): the
// kernel instantiation as text, NULL past the last kind.  Pure host arithmetic: without a GPU the CU count is 256, the MI355X's
extern "C" int quip_had_plan(const quip_had_problem* problems, int32_t count, int32_t planes, int64_t rows, int32_t n,
                             int32_t K, int32_t transpose, int32_t* out);
extern "C" const char* quip_had_plan_kind_name(int32_t kind);
// kernel 2 in quip_e8p_gemv_tuned = streaming-read probe (y is a 4-byte scratch)
// lane-ordered digit planes for the VALU integer GEMV (kernel 0); planes: 3*k + 16 bytes
extern "C" int quip_e8p_x_to_planes_laneorder(const void* x, void* planes, int32_t k, quip_stream_t stream);
// test hook (decode_probe.hip): every E8P12 code through the shared decode core of table mode `mode` (4 nibble | 16 | 24 | 32 byte
// tables), read back through the matrix core; codes: 64 tiles x 2 KB in item lane order, out: int8 [65536][8] = 4 w
extern "C" int quip_e8p_decode_probe(const void* grid, const void* codes, void* out, int32_t mode, quip_stream_t stream);
