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

from . import register_lib as _R

PAGE = _R._PAGE          # kPage == kChunkTile
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


def _check_exps(what, k_exp, v_exp):
    k_exp, v_exp = int(k_exp), int(v_exp)
    _R._need(F8_EXP_MIN <= k_exp <= F8_EXP_MAX and F8_EXP_MIN <= v_exp <= F8_EXP_MAX,
             f"{what}: exponents in [{F8_EXP_MIN}, {F8_EXP_MAX}]")
    return k_exp, v_exp


def _decode_paged(op, q, k, v, cos, sin, pos, table, kpool, vpool, workspace, window, exps=None):
    """both paged decode ops; exps (k_exp, v_exp): the one on uint8 pools, its entry takes them behind the stream"""
    B, heads, kvh, hd, max_len, _ = _R._check_attn(op, "batched", q, k, v, cos, sin, pos, kpool, vpool, table,
                                                   torch.float16 if exps is None else torch.uint8)
    more = () if exps is None else _check_exps(op, *exps)
    _R._check_attn_workspace(workspace, q, B, heads, hd)
    out = torch.empty_like(q)
    _R._attn_call("quip_" + op + ("_f16" if exps is None else ""), q, *_R._ptrs(q, k, v, cos, sin, pos, table, kpool, vpool, out),
                  B, heads, kvh, hd, max_len, kpool.shape[0], table.shape[1], 1.0 / math.sqrt(hd), int(window),
                  _R._ptr(workspace), _R._stream(q), *more)
    return out


def _ragged_paged(op, q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window, exps=None):
    """both paged ragged ops; exps as in _decode_paged"""
    rows, heads, kvh, hd, max_len, B = _R._check_attn(op, "ragged", q, k, v, cos, sin, pos, kpool, vpool, table,
                                                      torch.float16 if exps is None else torch.uint8)
    more = () if exps is None else _check_exps(op, *exps)
    n, slots, counts = _R._pack_segments(op, seg_slot, seg_rows, rows, B)
    out = torch.empty_like(q)
    _R._attn_call("quip_" + op + ("_f16" if exps is None else ""), q, *_R._ptrs(q, k, v, cos, sin, pos, table, kpool, vpool, out),
                  rows, heads, kvh, hd, max_len, B, kpool.shape[0], table.shape[1], ctypes.addressof(slots),
                  ctypes.addressof(counts), n, 1.0 / math.sqrt(hd), int(window), _R._stream(q), *more)
    return out


def _rope_attn_decode_paged_cuda(q, k, v, cos, sin, pos, table, kpool, vpool, workspace=None, window=0):
    """rope_attn_decode_batched with q (B, heads, hd), k / v (B, kv_heads, hd), pos (B,) and the caches behind `table`;
    row pos[b] of slot b is written -> (B, heads, hd) fp16"""
    return _decode_paged("rope_attn_decode_paged", q, k, v, cos, sin, pos, table, kpool, vpool, workspace, window)


def _rope_attn_ragged_paged_cuda(q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window=0):
    """rope_attn_ragged with the caches behind `table`: rows [pos[slot], pos[slot] + seg_rows[s]) of every named slot are
    written -> (rows, heads, hd) fp16"""
    return _ragged_paged("rope_attn_ragged_paged", q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window)


def _rope_attn_decode_paged_f8_cuda(q, k, v, cos, sin, pos, table, kpool, vpool, workspace=None, window=0, k_exp=0, v_exp=0):
    """rope_attn_decode_paged on uint8 pools of e4m3fn bytes at exponents (k_exp, v_exp) -> (B, heads, hd) fp16"""
    return _decode_paged("rope_attn_decode_paged_f8", q, k, v, cos, sin, pos, table, kpool, vpool, workspace, window,
                         (k_exp, v_exp))


def _rope_attn_ragged_paged_f8_cuda(q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window=0, k_exp=0,
                                    v_exp=0):
    """rope_attn_ragged_paged on uint8 pools of e4m3fn bytes at exponents (k_exp, v_exp) -> (rows, heads, hd) fp16"""
    return _ragged_paged("rope_attn_ragged_paged_f8", q, k, v, cos, sin, pos, seg_slot, seg_rows, table, kpool, vpool, window,
                         (k_exp, v_exp))


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
