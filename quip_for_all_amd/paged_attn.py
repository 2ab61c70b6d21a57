"""quip_lib::rope_attn_decode_paged and quip_lib::rope_attn_ragged_paged: the two batched attention launches
(rope_attn_decode_batched, rope_attn_ragged) on a PAGED KV cache (csrc/paged_attn.hip.h).

A page is PAGE = 64 consecutive positions of every KV head of one sequence.  kpool / vpool are (n_pages, kv_heads, 64, hd)
fp16, the block table is (B, max_pages) int32 on the device: entry [b][j] names the page of positions [64 j, 64 j + 64) of
slot b, -1 where none is assigned.  Only the address of a row changes, so outputs and cache rows are bit identical to
the contiguous op on the rows gathered through the table (`gather`).  An entry outside [0, n_pages) among the pages a
sequence / segment touches appends nothing for it and gives it NaN rows; the wrappers cannot see table contents (that
would be a host read) and do not try.  The caller guarantees that a page a slot appends to is referenced by that slot
only (paged_cache.PagePool keeps that invariant).

quip_lib::rope_attn_decode_paged_f8 / rope_attn_ragged_paged_f8: the same two launches on an FP8 cache.  The pools are
torch.uint8 (n_pages, kv_heads, 64, hd), one OCP e4m3fn byte per element; byte c of the K pool means e4m3fn(c) * 2^k_exp,
of the V pool e4m3fn(c) * 2^v_exp, the exponents integers in [-8, 7] (every code times 2^e is then an exact fp16 value).
Appended rows are quantised (saturating at +-448, NaN kept, round to nearest even) and used by the launch that appends
them as dequant(quant(row)) -- the round-trip rule of csrc/paged_attn.hip.h.  `quant_f8` / `dequant_f8` are the torch
model of the format (the tests' oracle)."""
import ctypes
import math

import torch

from . import capi
from . import register_lib as _R
from .ragged_attn import MAX_SEGMENTS

PAGE = 64          # kPage == kChunkTile
F8_EXP_MIN, F8_EXP_MAX = -8, 7

try:
    _R._lib.define("rope_attn_decode_paged(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, Tensor table, "
                   "Tensor(a!) kpool, Tensor(b!) vpool, Tensor(c!)? workspace, int window=0) -> Tensor")
    _R._lib.define("rope_attn_decode_paged_f8(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, Tensor table, "
                   "Tensor(a!) kpool, Tensor(b!) vpool, Tensor(c!)? workspace, int window=0, int k_exp=0, int v_exp=0) -> Tensor")
    _R._lib.define("rope_attn_ragged_paged_f8(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, int[] seg_slot, "
                   "int[] seg_rows, Tensor table, Tensor(a!) kpool, Tensor(b!) vpool, int window=0, int k_exp=0, int v_exp=0) "
                   "-> Tensor")
    _R._lib.define("rope_attn_ragged_paged(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, int[] seg_slot, "
                   "int[] seg_rows, Tensor table, Tensor(a!) kpool, Tensor(b!) vpool, int window=0) -> Tensor")
except RuntimeError:
    pass


def gather(pool, table):
    """the contiguous view of a paged cache: pool (n_pages, kv_heads, 64, hd), table (B, max_pages) of VALID entries
    -> (B, kv_heads, max_pages * 64, hd) (a copy; tests and debugging)"""
    B, mp = table.shape
    n, kvh, pg, hd = pool.shape
    return pool[table.long().reshape(-1)].view(B, mp, kvh, pg, hd).permute(0, 2, 1, 3, 4).reshape(B, kvh, mp * pg, hd)


def quant_f8(x, e):
    """the stored bytes (uint8) of x at exponent e: x * 2^-e in fp32, saturated to +-448, rounded to nearest even by
    torch's e4m3fn cast (which does not saturate, hence the clamp; clamp keeps NaN)"""
    return (x.float() * 2.0 ** -int(e)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def dequant_f8(b, e):
    """the fp16 values uint8 bytes b mean at exponent e (exact for e in [-8, 7])"""
    return (b.view(torch.float8_e4m3fn).float() * 2.0 ** int(e)).to(torch.float16)


def _check_paged(what, q, k, v, cos, sin, pos, table, kpool, vpool, rows_are_slots, pool_dtype=torch.float16):
    """dtype, shape, contiguity and device of everything both ops take -> (heads, hd, kvh, max_len, B, n_pages, max_pages)"""
    need = _R._need
    need(kpool.dtype == pool_dtype and vpool.dtype == pool_dtype,
         f"{what}: the pools must be {'fp16' if pool_dtype == torch.float16 else 'uint8 (e4m3fn bytes)'}")
    for t in (q, k, v):
        need(t.dtype == torch.float16, f"{what}: q, k, v must be fp16")
    for t in (q, k, v, kpool, vpool):
        need(t.is_contiguous() and t.is_cuda and t.device == q.device, f"{what}: contiguous tensors on one CUDA device")
    need(cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
         and cos.device == q.device and sin.device == q.device, "cos / sin must be contiguous float32 on q's device")
    need(q.dim() == 3 and kpool.dim() == 4 and table.dim() == 2,
         f"{what}: q (rows, heads, hd), pools (n_pages, kv_heads, {PAGE}, hd), table (B, max_pages)")
    rows, heads, hd = q.shape
    n_pages, kvh = kpool.shape[0], kpool.shape[1]
    B, max_pages = table.shape
    max_len = cos.shape[0]
    need(table.dtype == torch.int32 and table.is_contiguous() and table.device == q.device,
         "table must be a contiguous int32 (B, max_pages) tensor on q's device")
    need(pos.dtype == torch.int64 and tuple(pos.shape) == (B,) and pos.is_contiguous() and pos.device == q.device,
         "pos must be a contiguous int64 (B,) tensor on q's device")
    need(not rows_are_slots or rows == B, f"{what}: one q row per table row")
    need(tuple(k.shape) == (rows, kvh, hd) and tuple(v.shape) == (rows, kvh, hd)
         and tuple(kpool.shape) == (n_pages, kvh, PAGE, hd) and tuple(vpool.shape) == tuple(kpool.shape)
         and n_pages >= 1 and max_pages >= 1 and tuple(cos.shape) == (max_len, hd) and tuple(sin.shape) == (max_len, hd)
         and 1 <= max_len <= max_pages * PAGE, f"{what}: shape mismatch")
    return heads, hd, kvh, max_len, B, n_pages, max_pages


def _rope_attn_decode_paged_cuda(q, k, v, cos, sin, pos, table, kpool, vpool, workspace=None, window=0):
    """rope_attn_decode_batched with q (B, heads, hd), k / v (B, kv_heads, hd), pos (B,) and the caches behind `table`;
    row pos[b] of slot b is written -> (B, heads, hd) fp16"""
    heads, hd, kvh, max_len, B, n_pages, max_pages = _check_paged("rope_attn_decode_paged", q, k, v, cos, sin, pos, table,
                                                                  kpool, vpool, True)
    if workspace is not None:
        _R._need(workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == q.device
                 and workspace.numel() >= capi.lib().quip_rope_attn_batched_workspace_bytes(B, heads, hd),
                 "workspace: use rope_attn_batched_workspace(batch, heads, head_dim, device)")
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        capi.check(capi.lib().quip_rope_attn_decode_paged_f16(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), table.data_ptr(),
            kpool.data_ptr(), vpool.data_ptr(), out.data_ptr(), B, heads, kvh, hd, max_len, n_pages, max_pages,
            1.0 / math.sqrt(hd), int(window), _R._ptr(workspace), _R._stream(q)), "quip_rope_attn_decode_paged_f16")
    return out


def _rope_attn_ragged_paged_cuda(q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window=0):
    """rope_attn_ragged with the caches behind `table`: rows [pos[slot], pos[slot] + seg_rows[s]) of every named slot are
    written -> (rows, heads, hd) fp16"""
    need = _R._need
    heads, hd, kvh, max_len, B, n_pages, max_pages = _check_paged("rope_attn_ragged_paged", q, k, v, cos, sin, pos, table,
                                                                  kpool, vpool, False)
    rows = q.shape[0]
    seg_slot, seg_rows = [int(x) for x in seg_slot], [int(x) for x in seg_rows]
    n = len(seg_slot)
    need(1 <= n <= MAX_SEGMENTS and len(seg_rows) == n,
         f"rope_attn_ragged_paged: 1 .. {MAX_SEGMENTS} segments, one slot and one row count each")
    need(all(r >= 1 for r in seg_rows) and sum(seg_rows) == rows, "rope_attn_ragged_paged: seg_rows >= 1 that sum to q's rows")
    need(all(0 <= b < B for b in seg_slot) and len(set(seg_slot)) == n, "rope_attn_ragged_paged: distinct slots in [0, B)")
    slots, counts = (ctypes.c_int32 * n)(*seg_slot), (ctypes.c_int32 * n)(*seg_rows)
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        capi.check(capi.lib().quip_rope_attn_ragged_paged_f16(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), table.data_ptr(),
            kpool.data_ptr(), vpool.data_ptr(), out.data_ptr(), rows, heads, kvh, hd, max_len, B, n_pages, max_pages,
            ctypes.addressof(slots), ctypes.addressof(counts), n, 1.0 / math.sqrt(hd), int(window), _R._stream(q)),
            "quip_rope_attn_ragged_paged_f16")
    return out


def _check_exps(what, k_exp, v_exp):
    k_exp, v_exp = int(k_exp), int(v_exp)
    _R._need(F8_EXP_MIN <= k_exp <= F8_EXP_MAX and F8_EXP_MIN <= v_exp <= F8_EXP_MAX,
             f"{what}: exponents in [{F8_EXP_MIN}, {F8_EXP_MAX}]")
    return k_exp, v_exp


def _rope_attn_decode_paged_f8_cuda(q, k, v, cos, sin, pos, table, kpool, vpool, workspace=None, window=0, k_exp=0, v_exp=0):
    """rope_attn_decode_paged on uint8 pools of e4m3fn bytes at exponents (k_exp, v_exp) -> (B, heads, hd) fp16"""
    heads, hd, kvh, max_len, B, n_pages, max_pages = _check_paged("rope_attn_decode_paged_f8", q, k, v, cos, sin, pos, table,
                                                                  kpool, vpool, True, torch.uint8)
    k_exp, v_exp = _check_exps("rope_attn_decode_paged_f8", k_exp, v_exp)
    if workspace is not None:
        _R._need(workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == q.device
                 and workspace.numel() >= capi.lib().quip_rope_attn_batched_workspace_bytes(B, heads, hd),
                 "workspace: use rope_attn_batched_workspace(batch, heads, head_dim, device)")
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        capi.check(capi.lib().quip_rope_attn_decode_paged_f8(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), table.data_ptr(),
            kpool.data_ptr(), vpool.data_ptr(), out.data_ptr(), B, heads, kvh, hd, max_len, n_pages, max_pages,
            1.0 / math.sqrt(hd), int(window), _R._ptr(workspace), _R._stream(q), k_exp, v_exp),
            "quip_rope_attn_decode_paged_f8")
    return out


def _rope_attn_ragged_paged_f8_cuda(q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window=0, k_exp=0,
                                    v_exp=0):
    """rope_attn_ragged_paged on uint8 pools of e4m3fn bytes at exponents (k_exp, v_exp) -> (rows, heads, hd) fp16"""
    need = _R._need
    heads, hd, kvh, max_len, B, n_pages, max_pages = _check_paged("rope_attn_ragged_paged_f8", q, k, v, cos, sin, pos, table,
                                                                  kpool, vpool, False, torch.uint8)
    k_exp, v_exp = _check_exps("rope_attn_ragged_paged_f8", k_exp, v_exp)
    rows = q.shape[0]
    seg_slot, seg_rows = [int(x) for x in seg_slot], [int(x) for x in seg_rows]
    n = len(seg_slot)
    need(1 <= n <= MAX_SEGMENTS and len(seg_rows) == n,
         f"rope_attn_ragged_paged_f8: 1 .. {MAX_SEGMENTS} segments, one slot and one row count each")
    need(all(r >= 1 for r in seg_rows) and sum(seg_rows) == rows, "rope_attn_ragged_paged_f8: seg_rows >= 1 that sum to q's rows")
    need(all(0 <= b < B for b in seg_slot) and len(set(seg_slot)) == n, "rope_attn_ragged_paged_f8: distinct slots in [0, B)")
    slots, counts = (ctypes.c_int32 * n)(*seg_slot), (ctypes.c_int32 * n)(*seg_rows)
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        capi.check(capi.lib().quip_rope_attn_ragged_paged_f8(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), table.data_ptr(),
            kpool.data_ptr(), vpool.data_ptr(), out.data_ptr(), rows, heads, kvh, hd, max_len, B, n_pages, max_pages,
            ctypes.addressof(slots), ctypes.addressof(counts), n, 1.0 / math.sqrt(hd), int(window), _R._stream(q),
            k_exp, v_exp), "quip_rope_attn_ragged_paged_f8")
    return out


try:
    _R._lib.impl("rope_attn_decode_paged_f8", _rope_attn_decode_paged_f8_cuda, "CUDA")
    _R._lib.impl("rope_attn_ragged_paged_f8", _rope_attn_ragged_paged_f8_cuda, "CUDA")
    _R._reg_fake("rope_attn_decode_paged_f8",
                 lambda q, k, v, cos, sin, pos, table, kpool, vpool, workspace=None, window=0, k_exp=0, v_exp=0:
                 torch.empty_like(q))
    _R._reg_fake("rope_attn_ragged_paged_f8",
                 lambda q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window=0, k_exp=0, v_exp=0:
                 torch.empty_like(q))
except RuntimeError:
    pass

try:
    _R._lib.impl("rope_attn_decode_paged", _rope_attn_decode_paged_cuda, "CUDA")
    _R._lib.impl("rope_attn_ragged_paged", _rope_attn_ragged_paged_cuda, "CUDA")
    _R._reg_fake("rope_attn_decode_paged",
                 lambda q, k, v, cos, sin, pos, table, kpool, vpool, workspace=None, window=0: torch.empty_like(q))
    _R._reg_fake("rope_attn_ragged_paged",
                 lambda q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window=0: torch.empty_like(q))
except RuntimeError:
    pass
