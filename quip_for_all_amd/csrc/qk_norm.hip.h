// Per-head RMSNorm of q and k between the projections and the rotary embedding (Qwen3: self_attn.q_norm / k_norm, one
// (HD,) weight each, shared by the heads).  Part of decode_glue.hip's translation unit.  Two ways to get it:
//
// qk_norm_rows_kernel: the stand-alone launch.  Every head of q (rows, heads * HD) and of k (rows, kv_heads * HD) is
// normalised in place, both tensors in ONE launch.  A head is handled by its HD / 8 lanes (8 dims, 16 bytes per lane, as
// everywhere in attn_query.hip.h): one load, inv_rms, norm8, one store.  Head g of the launch -- rows * (heads +
// kv_heads) of them, row-major, a row's q heads before its k heads -- belongs to lane group g; 256 threads per workgroup.
// With HD = 64 two heads share a 16-lane row: sum16_xor<8> adds inside the aligned 8 lanes only, so a head's result does
// not depend on its neighbour.  Lane groups past the last head compute on the last head and store nothing.
//
// The kNorm instantiations of rope_attn_decode_kernel (QkNormArgs, decode_glue.hip): q and the new k row normalised in
// registers between the load and the rotation -- the bs = 1 launch (window and split mode included) and the contiguous
// batched launch.  Same primitives, so the same bits as this launch followed by the plain one, in the output and in the
// appended cache row.  The other attention launches (padded start, paged, fp8, chunk, ragged, _z) take this launch in
// front.
#pragma once
#include "attn_query.hip.h"
#include "launch.hip.h"
#include "quip_device.hip.h"

namespace quip {
namespace {

template <int HD>
__global__ __launch_bounds__(256) void qk_norm_rows_kernel(f16* __restrict__ q, f16* __restrict__ k,
                                                           const f16* __restrict__ qw, const f16* __restrict__ kw,
                                                           int heads, int kv_heads, long long total, float eps) {
  constexpr int LPK = HD / 8;
  const long long g = (long long)blockIdx.x * (256 / LPK) + threadIdx.x / LPK;
  const bool live = g < total;
  const long long gc = live ? g : total - 1;
  const int per_row = heads + kv_heads;
  const long long row = gc / per_row;
  const int hh = (int)(gc - row * per_row);
  const bool is_q = hh < heads;
  f16* vec = is_q ? q + ((size_t)row * heads + hh) * HD : k + ((size_t)row * kv_heads + (hh - heads)) * HD;
  const f16* w = is_q ? qw : kw;
  const int d0 = (threadIdx.x % LPK) * 8;
  float a[8];
  attn::unpack8h(*reinterpret_cast<const uint4*>(vec + d0), a);
  const float r = attn::inv_rms<HD>(a, eps);
  attn::norm8(a, r, w + d0);
  if (live) {
    uint4 o;
    o.x = pack_f16(a[0], a[1]); o.y = pack_f16(a[2], a[3]);
    o.z = pack_f16(a[4], a[5]); o.w = pack_f16(a[6], a[7]);
    *reinterpret_cast<uint4*>(vec + d0) = o;
  }
}

// decode_launch (decode_glue.hip) on QkNormArgs<AttnArgs>: the grid rule and the workspace of the launch without the norm
template <bool SEQ>
int decode_qknorm_launch(const AttnIO& io, const AttnShape& s, const AttnQkNorm& norm, int batch, hipStream_t stream,
                         void* workspace) {
  if ((SEQ && !batch_ok(batch)) || !attn_shape_ok(s)) return QUIP_ERR_BAD_SHAPE;
  auto a = make_attn_args_as<QkNormArgs<AttnArgs>>(io, s);
  a.qw = reinterpret_cast<const f16*>(norm.qw);
  a.kw = reinterpret_cast<const f16*>(norm.kw);
  a.eps = norm.eps;
  return decode_launch<SEQ>(a, batch, s.head_dim, s.max_len, 0, stream, workspace);
}

}  // namespace

int qk_norm_rows_launch(void* q, void* k, const void* qw, const void* kw, int64_t rows, int heads, int kv_heads,
                        int head_dim, float eps, hipStream_t stream) {
  if (rows < 1 || heads < 1 || kv_heads < 1 || heads > 65536 || kv_heads > 65536) return QUIP_ERR_BAD_SHAPE;
  if (head_dim != 64 && head_dim != 128) return QUIP_ERR_UNSUPPORTED;
  const long long total = (long long)rows * (heads + kv_heads);
  const int per_wg = 256 / (head_dim / 8);
  const long long blocks = (total + per_wg - 1) / per_wg;
  if (blocks > 0x7fffffffll) return QUIP_ERR_BAD_SHAPE;
  f16* qp = reinterpret_cast<f16*>(q);
  f16* kp = reinterpret_cast<f16*>(k);
  const f16* qwp = reinterpret_cast<const f16*>(qw);
  const f16* kwp = reinterpret_cast<const f16*>(kw);
  if (head_dim == 128)
    return launch<qk_norm_rows_kernel<128>>(dim3((unsigned)blocks), dim3(256), 0, stream, qp, kp, qwp, kwp, heads, kv_heads,
                                            total, eps);
  return launch<qk_norm_rows_kernel<64>>(dim3((unsigned)blocks), dim3(256), 0, stream, qp, kp, qwp, kwp, heads, kv_heads, total,
                                         eps);
}

int rope_attn_decode_qknorm_launch(const AttnIO& io, const AttnShape& s, const AttnQkNorm& norm, hipStream_t stream,
                                   void* workspace) {
  return decode_qknorm_launch<false>(io, s, norm, 1, stream, workspace);
}

int rope_attn_decode_batched_qknorm_launch(const AttnIO& io, const AttnShape& s, const AttnQkNorm& norm, hipStream_t stream,
                                           void* workspace) {
  return decode_qknorm_launch<true>(io, s, norm, s.batch, stream, workspace);
}

}  // namespace quip
