"""quip_lib::rope_attn_chunk: rotary embedding, KV-cache append and causal attention for a chunk of prompt rows at
positions [pos, pos + rows) against cache rows [0, pos + rows), one launch (csrc/chunk_attn.hip.h).

The prompt-side counterpart of rope_attn_decode: q / out are token major (rows, heads, hd), the position is a device
scalar the launch reads itself, so a captured call serves every start position.  LlamaDecoder.extend() builds on it."""
import math

import torch

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
    rows, heads, kvh, hd, max_len, _ = _R._check_attn("rope_attn_chunk", "chunk", q, k, v, cos, sin, pos, kcache, vcache)
    out = torch.empty_like(q)
    _R._attn_call("quip_rope_attn_chunk_f16", q, *_R._ptrs(q, k, v, cos, sin, pos, kcache, vcache, out), rows, heads, kvh, hd,
                  max_len, 1.0 / math.sqrt(hd), int(window), _R._stream(q))
    return out


try:
    _R._lib.impl("rope_attn_chunk", _rope_attn_chunk_cuda, "CUDA")
    _R._reg_fake("rope_attn_chunk", lambda q, k, v, cos, sin, pos, kcache, vcache, window=0: torch.empty_like(q))
except RuntimeError:
    pass
