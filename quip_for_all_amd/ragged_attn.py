"""quip_lib::rope_attn_ragged: quip_lib::rope_attn_chunk for a ragged batch of chunks -- several slots of a batched KV cache
continued in one launch (csrc/ragged_attn.hip.h).

The rows of q / k / v are segments of consecutive rows; segment s has seg_rows[s] rows and continues slot seg_slot[s] of
the (B, kv_heads, max_len, hd) caches at the position the launch reads from pos[seg_slot[s]].  Per segment the result is
bit identical to rope_attn_chunk on that segment alone; slots must be distinct.  The segment table is host data (it
travels in the kernel arguments), the positions stay on the device.  BatchDecoder.extend_slots() builds on it."""
import ctypes
import math

import torch

from . import capi
from . import register_lib as _R

MAX_SEGMENTS = 32          # QUIP_RAGGED_MAX_SEGMENTS

try:
    _R._lib.define("rope_attn_ragged(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, int[] seg_slot, "
                   "int[] seg_rows, Tensor(a!) kcache, Tensor(b!) vcache, int window=0) -> Tensor")
except RuntimeError:
    pass


def _rope_attn_ragged_cuda(q, k, v, cos, sin, pos, seg_slot, seg_rows, kcache, vcache, window=0):
    """q (rows, heads, hd), k / v (rows, kv_heads, hd) fp16 (k pre-rope); cos / sin (max_len, hd) fp32; pos (B,) int64 on
    the device; seg_slot / seg_rows: python ints, sum(seg_rows) == rows, distinct slots in [0, B); kcache / vcache
    (B, kv_heads, max_len, hd) fp16, rows [pos[slot], pos[slot] + seg_rows[s]) of every named slot are written
    -> (rows, heads, hd) fp16"""
    need = _R._need
    for t in (q, k, v, kcache, vcache):
        need(t.dtype == torch.float16 and t.is_contiguous() and t.is_cuda and t.device == q.device,
             "rope_attn_ragged: fp16 contiguous tensors on one CUDA device")
    need(cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
         and cos.device == q.device and sin.device == q.device, "cos / sin must be contiguous float32 on q's device")
    need(q.dim() == 3 and kcache.dim() == 4, "rope_attn_ragged: q (rows, heads, hd), caches (B, kv_heads, max_len, hd)")
    rows, heads, hd = q.shape
    B, kvh, max_len = kcache.shape[0], kcache.shape[1], kcache.shape[2]
    need(pos.dtype == torch.int64 and tuple(pos.shape) == (B,) and pos.is_contiguous() and pos.device == q.device,
         "pos must be a contiguous int64 (B,) tensor on q's device")
    need(tuple(k.shape) == (rows, kvh, hd) and tuple(v.shape) == (rows, kvh, hd) and tuple(kcache.shape) == (B, kvh, max_len, hd)
         and tuple(vcache.shape) == tuple(kcache.shape) and tuple(cos.shape) == (max_len, hd)
         and tuple(sin.shape) == (max_len, hd), "rope_attn_ragged: shape mismatch")
    seg_slot, seg_rows = [int(x) for x in seg_slot], [int(x) for x in seg_rows]
    n = len(seg_slot)
    need(1 <= n <= MAX_SEGMENTS and len(seg_rows) == n, f"rope_attn_ragged: 1 .. {MAX_SEGMENTS} segments, one slot and one row count each")
    need(all(r >= 1 for r in seg_rows) and sum(seg_rows) == rows, "rope_attn_ragged: seg_rows >= 1 that sum to q's rows")
    need(all(0 <= b < B for b in seg_slot) and len(set(seg_slot)) == n, "rope_attn_ragged: distinct slots in [0, B)")
    slots, counts = (ctypes.c_int32 * n)(*seg_slot), (ctypes.c_int32 * n)(*seg_rows)
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        capi.check(capi.lib().quip_rope_attn_ragged_f16(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(),
            kcache.data_ptr(), vcache.data_ptr(), out.data_ptr(), rows, heads, kvh, hd, max_len, B,
            ctypes.addressof(slots), ctypes.addressof(counts), n, 1.0 / math.sqrt(hd), int(window), _R._stream(q)),
            "quip_rope_attn_ragged_f16")
    return out


try:
    _R._lib.impl("rope_attn_ragged", _rope_attn_ragged_cuda, "CUDA")
    _R._reg_fake("rope_attn_ragged",
                 lambda q, k, v, cos, sin, pos, seg_slot, seg_rows, kcache, vcache, window=0: torch.empty_like(q))
except RuntimeError:
    pass
