"""quip_lib::rope_attn_chunk: rotary embedding, KV-cache append and causal attention for a chunk of prompt rows at
positions [pos, pos + rows) against cache rows [0, pos + rows), one launch (csrc/chunk_attn.hip.h).

The prompt-side counterpart of rope_attn_decode: q / out are token major (rows, heads, hd), the position is a device
scalar the launch reads itself, so a captured call serves every start position.  LlamaDecoder.extend() builds on it."""
import math

import torch

from . import capi
from . import register_lib as _R

try:
    _R._lib.define("rope_attn_chunk(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, "
                   "Tensor(a!) kcache, Tensor(b!) vcache, int window=0) -> Tensor")
except RuntimeError:
    pass


def _rope_attn_chunk_cuda(q, k, v, cos, sin, pos, kcache, vcache, window=0):
    """q (rows, heads, hd), k / v (rows, kv_heads, hd) fp16 (k pre-rope); cos / sin (max_len, hd) fp32; pos int64 device
    scalar (position of row 0); kcache / vcache (kv_heads, max_len, hd) fp16, rows [pos, pos + rows) are written
    -> (rows, heads, hd) fp16"""
    need = _R._need
    for t in (q, k, v, kcache, vcache):
        need(t.dtype == torch.float16 and t.is_contiguous() and t.is_cuda and t.device == q.device,
             "rope_attn_chunk: fp16 contiguous tensors on one CUDA device")
    need(cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
         and cos.device == q.device and sin.device == q.device, "cos / sin must be contiguous float32 on q's device")
    need(q.dim() == 3 and kcache.dim() == 3, "rope_attn_chunk: q (rows, heads, hd), caches (kv_heads, max_len, hd)")
    rows, heads, hd = q.shape
    kvh, max_len = kcache.shape[0], kcache.shape[1]
    need(rows >= 1, "rope_attn_chunk: at least one row")
    need(pos.dtype == torch.int64 and pos.numel() == 1 and pos.device == q.device,
         "pos must be an int64 scalar tensor on q's device")
    need(tuple(k.shape) == (rows, kvh, hd) and tuple(v.shape) == (rows, kvh, hd) and tuple(kcache.shape) == (kvh, max_len, hd)
         and tuple(vcache.shape) == tuple(kcache.shape) and tuple(cos.shape) == (max_len, hd)
         and tuple(sin.shape) == (max_len, hd), "rope_attn_chunk: shape mismatch")
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        capi.check(capi.lib().quip_rope_attn_chunk_f16(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(),
            kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), rows, heads, kvh, hd, max_len, 1.0 / math.sqrt(hd),
            int(window), _R._stream(q)), "quip_rope_attn_chunk_f16")
    return out


try:
    _R._lib.impl("rope_attn_chunk", _rope_attn_chunk_cuda, "CUDA")
    _R._reg_fake("rope_attn_chunk", lambda q, k, v, cos, sin, pos, kcache, vcache, window=0: torch.empty_like(q))
except RuntimeError:
    pass
