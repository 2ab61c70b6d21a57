"""quip_lib::rope_attn_ragged: quip_lib::rope_attn_chunk for a ragged batch of chunks -- several slots of a batched KV cache
continued in one launch (csrc/ragged_attn.hip.h).

The rows of q / k / v are segments of consecutive rows; segment s has seg_rows[s] rows and continues slot seg_slot[s] of
the (B, kv_heads, max_len, hd) caches at the position the launch reads from pos[seg_slot[s]].  Per segment the result is
bit identical to rope_attn_chunk on that segment alone; slots must be distinct.  The segment table is host data (it
travels in the kernel arguments), the positions stay on the device.  BatchDecoder.extend_slots() builds on it."""
import ctypes
import math

import torch

from . import register_lib as _R

MAX_SEGMENTS = _R._MAX_SEGMENTS          # QUIP_RAGGED_MAX_SEGMENTS

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
    rows, heads, kvh, hd, max_len, B = _R._check_attn("rope_attn_ragged", "ragged", q, k, v, cos, sin, pos, kcache, vcache)
    n, slots, counts = _R._pack_segments("rope_attn_ragged", seg_slot, seg_rows, rows, B)
    out = torch.empty_like(q)
    _R._attn_call("quip_rope_attn_ragged_f16", q, *_R._ptrs(q, k, v, cos, sin, pos, kcache, vcache, out), rows, heads, kvh, hd,
                  max_len, B, ctypes.addressof(slots), ctypes.addressof(counts), n, 1.0 / math.sqrt(hd), int(window),
                  _R._stream(q))
    return out


try:
    _R._lib.impl("rope_attn_ragged", _rope_attn_ragged_cuda, "CUDA")
    _R._reg_fake("rope_attn_ragged",
                 lambda q, k, v, cos, sin, pos, seg_slot, seg_rows, kcache, vcache, window=0: torch.empty_like(q))
except RuntimeError:
    pass
